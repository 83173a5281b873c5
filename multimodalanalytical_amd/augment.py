"""Training-set augmentation of the `augment` config group (reference data/augmentations.py, applied to the train split at
data/datasets.py:377-378) on the device.

The reference expands the train set on the CPU, one `datasets.map` call per row.  Here a host planner turns the composed
`augment` group into a row map over the expanded set -- source row `src[r]` and, per augmented spectrum modality, an op
index `op[r]` into a small op table -- and `afm_spectra_augment` produces the spectra of those rows in one launch:

    expanded row order   [train rows] + [one block per `augmentations` entry, in config order] + [augment_data_path rows]
    inside a block       every source row in turn, expanded in place: augment_fns order, then sigma / shift order
    other columns        duplicated (index_select on src), text modalities included

Two ways to use the plan: `materialise` writes the expanded train shard (what the step count, the PatchPreprocessor statistics,
ShardLoader and MixtureLoader then see), `OnTheFly` keeps the table 1x and produces each micro-batch's rows from their
(src, op) pairs -- the same kernel on the same pairs, so the batches are the materialised ones bit for bit.

Stated differences from the reference: `augment_data_path` names a directory holding a pre-tokenised `train.pt` in this
repo's shard format (cli/training.py docstring) instead of a `datasets.load_from_disk` directory; train rows without a spectrum
(`present == 0`) are refused, where the reference fails on the `None`; `smiles_aug` (RDKit random SMILES) is refused.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops

TRUNCATE = 4.0       # gaussian_filter1d's default
FN_PARAMS = {"smooth": ("sigmas",), "horizontal": ("n_augments",)}


def gaussian_half_kernel(sigma: float, truncate: float = TRUNCATE):
    """(radius, w_0 .. w_radius) of scipy.ndimage.gaussian_filter1d(sigma): _gaussian_kernel1d's exp(-0.5 / sigma^2 * x^2)
    normalised by its sum, the same numpy calls in the same order, so the weights are SciPy's to the bit (the kernel is
    symmetric)."""
    sd = float(sigma)
    if not sd > 0.0:
        raise ValueError(f"smooth: sigma must be > 0, got {sigma!r}")
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[::-1][radius:].copy()        # correlate1d's fw[0 .. radius] of the reversed weights


@dataclass
class AugmentPlan:
    src: np.ndarray                   # (M,) int64: source row of every expanded row (into train rows + extra rows)
    op: Dict[str, np.ndarray]         # modality -> (M,) int32 index into op_table (0 = copy)
    op_table: np.ndarray              # (K, 3) int32 {kind, a, b} (include/afm_hip.h, afm_spectra_augment)
    weights: np.ndarray               # fp64 Gaussian half kernels, concatenated
    n_train: int
    n_extra: int = 0
    on_the_fly: bool = False
    blocks: List[int] = field(default_factory=list)    # rows per augmentations entry

    @property
    def rows(self) -> int:
        return int(self.src.shape[0])


def spectrum_modality(data_cfg: Dict[str, Any], column: str) -> str:
    """The modality whose `column` is `column` (`augment_column` names a dataset column, data[m].column maps it)."""
    for m, mc in data_cfg.items():
        if mc.get("column") == column and not mc.get("alignment"):
            if mc.get("type") != "1D_patches":
                raise NotImplementedError(f"augment_column {column!r} is modality {m!r} of type {mc.get('type')!r}: only 1D_patches "
                                          f"spectra are augmented on the device")
            return m
    raise KeyError(f"augment_column {column!r} is not the column of any modality of the data config "
                   f"({sorted(str(mc.get('column')) for mc in data_cfg.values())})")


def shard_rows(shard) -> int:
    first = next(iter(shard["data"].values()))
    return int(next(iter(first.values())).shape[0])


def plan_augmentation(augment_cfg: Optional[Dict[str, Any]], data_cfg: Dict[str, Any], shard, n_extra: int = 0) -> Optional[AugmentPlan]:
    """The row map of `augment(train, augment_config)` (augmentations.py:57-107) for the train `shard`, `n_extra` rows of
    augment_data_path appended.  None when the group changes nothing (no_augment, or no dict at all)."""
    if not isinstance(augment_cfg, dict):
        return None
    entries = augment_cfg.get("augmentations")
    entries = list(entries) if isinstance(entries, list) else []
    if not entries and not n_extra:
        return None
    n = shard_rows(shard)
    table = [[0, 0, 0]]                 # op 0: copy
    weights: List[np.ndarray] = []
    woff = 0
    src = [np.arange(n, dtype=np.int64)]
    op: Dict[str, List[np.ndarray]] = {}
    blocks = []
    for e in entries:
        fns = dict(e.get("augment_fns") or {})
        for name, params in fns.items():
            if name == "smiles_aug":
                raise NotImplementedError("smiles_aug needs RDKit random SMILES (Chem.MolToSmiles(doRandom=True)), which this "
                                          "build does not carry: augment text columns off-line into augment_data_path instead")
            if name not in FN_PARAMS:
                raise KeyError(f"unknown augmentation {name!r} (known: {sorted(FN_PARAMS)} and smiles_aug)")
            unknown = set(params or {}) - set(FN_PARAMS[name])
            if unknown:
                raise TypeError(f"augmentation {name!r} got unexpected parameters {sorted(unknown)}")
        m = spectrum_modality(data_cfg, e["augment_column"])
        if m not in shard["data"] or "spectra" not in shard["data"][m]:
            raise KeyError(f"modality {m!r} (augment_column {e['augment_column']!r}) is missing from the train shard")
        d = shard["data"][m]
        L = int(d["spectra"].shape[1])
        if "present" in d and not bool(torch.as_tensor(d["present"]).bool().all()):
            raise ValueError(f"{int((~torch.as_tensor(d['present']).bool()).sum())} train rows of {m!r} have no spectrum "
                             f"(present == 0): they cannot be augmented")
        ids = []
        for name, params in fns.items():
            params = dict(params or {})
            if name == "smooth":
                for sigma in params["sigmas"]:
                    radius, w = gaussian_half_kernel(sigma)
                    table.append([ops.AUG_GAUSS, radius, woff])
                    weights.append(w)
                    woff += w.size
                    ids.append(len(table) - 1)
            else:
                k = int(params.get("n_augments", 2))     # horizontal_shift_augment's default
                if k < 1 or L % k == 0 or L // k < 2:
                    raise ValueError(f"horizontal n_augments={k} on spectra of length {L}: the shifted slice has {-(-L // k) - 1} "
                                     f"points against {L // k} knots (the reference's interp1d raises the same ValueError "
                                     f"whenever L % n_augments == 0)")
                for i in range(k):
                    table.append([ops.AUG_HSHIFT, k, i])
                    ids.append(len(table) - 1)
        per = len(ids)
        if per == 0:
            continue
        src.append(np.repeat(np.arange(n, dtype=np.int64), per))
        col = np.tile(np.asarray(ids, dtype=np.int32), n)
        op.setdefault(m, [np.zeros(n, dtype=np.int32)] + [np.zeros(b, dtype=np.int32) for b in blocks])
        for mm in op:
            op[mm].append(col if mm == m else np.zeros(n * per, dtype=np.int32))
        blocks.append(n * per)
    if n_extra:
        src.append(np.arange(n, n + n_extra, dtype=np.int64))
        for mm in op:
            op[mm].append(np.zeros(n_extra, dtype=np.int32))
    return AugmentPlan(src=np.concatenate(src), op={m: np.concatenate(v) for m, v in op.items()},
                       op_table=np.asarray(table, dtype=np.int32).reshape(-1, 3),
                       weights=np.concatenate(weights) if weights else np.zeros(0, dtype=np.float64),
                       n_train=n, n_extra=n_extra, on_the_fly=bool(augment_cfg.get("on_the_fly", False)), blocks=blocks)


def load_extra(path, meta) -> Dict[str, Any]:
    """The pre-tokenised `train.pt` of `augment_data_path` (this repo's shard format), checked against the train shard's meta."""
    import os
    p = os.path.join(str(path), "train.pt")
    if not os.path.isfile(p):
        raise FileNotFoundError(f"augment_data_path {path!r}: {p} not found (a directory holding a pre-tokenised train.pt in the "
                                f"shard format of cli/training.py)")
    extra = torch.load(p, map_location="cpu", weights_only=False)
    for m, mm in meta.items():
        got = extra.get("meta", {}).get(m)
        if got is None or int(got["vocab_size"]) != int(mm["vocab_size"]) or int(got.get("pad_token_id", 0)) != int(mm.get("pad_token_id", 0)):
            raise ValueError(f"augment_data_path {path!r}: meta of modality {m!r} ({got}) differs from the train shard's ({mm})")
    return extra


def base_data(shard, extra=None) -> Dict[str, Dict[str, torch.Tensor]]:
    """The 1x table: the train shard's tensors with the extra rows appended (same modalities, keys and row shapes)."""
    if extra is None:
        return shard["data"]
    out = {}
    for m, d in shard["data"].items():
        e = extra["data"].get(m)
        if e is None or set(e) != set(d):
            raise ValueError(f"augment_data_path: modality {m!r} has keys {None if e is None else sorted(e)}, the train shard {sorted(d)}")
        out[m] = {}
        for k, v in d.items():
            if tuple(e[k].shape[1:]) != tuple(v.shape[1:]) or e[k].dtype != v.dtype:
                raise ValueError(f"augment_data_path: {m}.{k} is {tuple(e[k].shape)} {e[k].dtype}, the train shard's {tuple(v.shape)} {v.dtype}")
            out[m][k] = torch.cat([v, e[k].to(v.device)])
    return out


class OnTheFly:
    """A plan on the device: the rows of any subset of the expanded index space, produced from their (src, op) pairs."""

    def __init__(self, plan: AugmentPlan, device):
        self.plan = plan
        self.rows = plan.rows
        self.src = torch.from_numpy(plan.src).to(device)
        self.op = {m: torch.from_numpy(v).to(device) for m, v in plan.op.items()}
        self.weights = torch.from_numpy(plan.weights).to(device)

    def gather(self, data: Dict[str, Dict[str, torch.Tensor]], idx: torch.Tensor) -> Dict[str, Dict[str, torch.Tensor]]:
        s = self.src.index_select(0, idx)
        out = {}
        for m, d in data.items():
            out[m] = {}
            for k, v in d.items():
                if k == "spectra" and m in self.op:
                    out[m][k] = ops.spectra_augment(v.contiguous(), s, self.op[m].index_select(0, idx), self.plan.op_table, self.weights)
                else:
                    out[m][k] = v.index_select(0, s)
        return out


def materialise(shard, plan: AugmentPlan, device, extra=None) -> Dict[str, Any]:
    """The expanded train shard, on the device: one afm_spectra_augment launch per augmented modality over all M rows."""
    data = {m: {k: v.to(device) for k, v in d.items()} for m, d in base_data(shard, extra).items()}
    rows = OnTheFly(plan, device).gather(data, torch.arange(plan.rows, device=device))
    return {"meta": shard["meta"], "data": rows}
