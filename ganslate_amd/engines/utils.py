"""init_engine (ganslate/engines/utils.py:14-22): the training and test engines (the Inferer is out of scope)."""
from ..utils import communication
from ..utils.builders import build_conf
from .trainer import Trainer
from .validator import Tester

ENGINES = {"train": Trainer, "test": Tester}


def init_engine(mode, omegaconf_args):
    if mode not in ENGINES:
        raise NotImplementedError(f"engine `{mode}` is outside the scope of the MI355X build (train and test only)")
    communication.init_distributed()
    conf = build_conf(omegaconf_args)
    return ENGINES[mode](conf)
