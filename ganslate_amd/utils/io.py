"""`_target_` resolution (ganslate/utils/io.py:73-76). Reference YAMLs name classes under `ganslate.*`; those
resolve to this package's counterparts, so the YAMLs run unchanged."""
import collections.abc
import importlib

import torch


def import_attr(module_attr: str):
    module, attr = module_attr.rsplit(".", 1)
    if module == "ganslate" or module.startswith("ganslate."):
        module = "ganslate_amd" + module[len("ganslate"):]
    return getattr(importlib.import_module(module), attr)


def mkdirs(*paths):
    from pathlib import Path
    for p in paths:
        Path(p).mkdir(parents=True, exist_ok=True)


def decollate(data, batch_size=None):
    """A collated batch (a dict, as a DataLoader's default collate builds it) back into a list of per-sample dicts
    (ganslate/utils/io.py:88-151, MONAI's decollate_batch): tensors are indexed along the batch axis, one-element tensors
    become Python scalars, lists of per-sample values (strings, e.g. file names) give their element, nested dicts and
    lists of sequences recurse. The batch size is that of the first tensor when not given."""
    if not isinstance(data, dict):
        raise RuntimeError("Only currently implemented for dictionary data (might be trivial to adapt).")
    if batch_size is None:
        batch_size = next((v.shape[0] for v in data.values() if isinstance(v, torch.Tensor)), None)
    if batch_size is None:
        raise RuntimeError("Couldn't determine batch size, please specify as argument.")

    def single(t):
        return t if t.numel() > 1 else t.item()

    def is_sequence(x):
        if isinstance(x, torch.Tensor):
            return x.dim() > 0
        return isinstance(x, collections.abc.Iterable) and not isinstance(x, str)

    def pick(value, idx):
        if isinstance(value, dict):
            return {k: pick(v, idx) for k, v in value.items()}
        if isinstance(value, torch.Tensor):
            return single(value[idx])
        if isinstance(value, list):
            if not value:
                return value
            if isinstance(value[0], torch.Tensor):
                return [single(v[idx]) for v in value]
            if is_sequence(value[0]):
                return [pick(v, idx) for v in value]
            return value[idx]
        raise TypeError(f"Not sure how to de-collate type: {type(value)}")

    return [{k: pick(v, idx) for k, v in data.items()} for idx in range(batch_size)]
