"""init_engine (ganslate/engines/utils.py:14-22): the training, test and inference engines. An engine whose section the
config does not have (`val`, `test` and `infer` are optional, configs/config.py) has nothing to run: that is refused here
with NotImplementedError, the error of an unknown engine name, before anything is built (the reference fails later, on an
attribute of `None`)."""
from ..utils import communication
from ..utils.builders import build_conf
from .inferer import Inferer
from .trainer import Trainer
from .validator import Tester

ENGINES = {"train": Trainer, "test": Tester, "infer": Inferer}


def init_engine(mode, omegaconf_args):
    if mode not in ENGINES:
        raise NotImplementedError(f"engine `{mode}` is outside the scope of the MI355X build (train, test and infer)")
    communication.init_distributed()
    conf = build_conf(omegaconf_args)
    if conf.get(mode) is None:
        raise NotImplementedError(f"engine `{mode}`: the config has no `{mode}` section, so there is nothing for it to run")
    return ENGINES[mode](conf)
