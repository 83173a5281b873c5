"""CPU: the `augment` config group (reference configs/augment/ir/*.yaml, data/augmentations.py) -- configs, the host planner's
row map and op table against the reference's own augment() (tests/golden/augment.npz, tools/make_augment_goldens.py), the
step count of the expanded set, the refusals, and the numpy restatement of the two ops against the golden outputs."""
import os

import numpy as np
import pytest
import torch

from tests import augment_numpy as A
from tests import golden_io as G

from multimodalanalytical_amd import augment as AU
from multimodalanalytical_amd.cli import training as T
from multimodalanalytical_amd.config import compose
from multimodalanalytical_amd.trainer import calculate_training_steps

GOLD = G.load("augment")
META = GOLD["meta"]
CASES = sorted(META["cases"])
# the golden tables' columns: ir_spectra (augmented), hnmr_spectra (a second spectrum column, never augmented), smiles (text)
DATA = {"IR": {"type": "1D_patches", "column": "ir_spectra", "target": False},
        "HNMR": {"type": "1D_patches", "column": "hnmr_spectra", "target": False},
        "Smiles": {"type": "text", "column": "smiles", "target": True}}


def _shard(tag):
    inp = GOLD[tag]["in"]
    data = {"IR": {"spectra": inp["ir_spectra"]}}
    if "hnmr_spectra" in inp:
        data["HNMR"] = {"spectra": inp["hnmr_spectra"]}
    return {"meta": {}, "data": data}


def _cfg(*overrides):
    return compose(T.DEFAULT_CONFIG_DIR, "config_train", list(overrides))


@pytest.mark.parametrize("name", ["smooth", "horizontal", "combined", "smiles", "pseudo"])
def test_augment_configs_compose_to_the_references(name):
    assert _cfg(f"augment=ir/{name}")["augment"] == META["reference_configs"][name]


def test_no_augment_changes_nothing():
    cfg = _cfg()
    assert cfg["augment"] == {"augment_data_path": None, "augmentations": None}
    train = {"meta": {}, "data": {"IR": {"spectra": torch.zeros(4, 1791)}}}
    assert AU.plan_augmentation(cfg["augment"], cfg["data"], train) is None
    got, sample = T.augment_train(cfg, train, "cpu")
    assert got is train and sample is None


@pytest.mark.parametrize("tag", CASES)
def test_planner_row_map_matches_the_reference_order(tag):
    case = META["cases"][tag]
    plan = AU.plan_augmentation(case["augment"], DATA, _shard(tag))
    src = GOLD[tag]["src"].numpy()
    assert plan.rows == src.size and np.array_equal(plan.src, src)
    n = case["rows"]
    assert np.array_equal(plan.src[:n], np.arange(n)) and not plan.op["IR"][:n].any()       # the originals come first, copied
    assert sum(plan.blocks) == plan.rows - n and "HNMR" not in plan.op
    kinds = plan.op_table[plan.op["IR"], 0]
    assert (kinds[n:] != A.COPY).all()
    # op order inside a block: augment_fns order, then sigma / shift order, repeated per source row
    per = plan.blocks[0] // n
    first = [tuple(r) for r in plan.op_table[plan.op["IR"][n:n + per]]]
    want = []
    for fn, p in case["augment"]["augmentations"][0]["augment_fns"].items():
        want += ([(A.GAUSS, AU.gaussian_half_kernel(s)[0]) for s in p["sigmas"]] if fn == "smooth" else
                 [(A.HSHIFT, p["n_augments"], i) for i in range(p["n_augments"])])
    assert [f[:len(w)] for f, w in zip(first, want)] == want


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_outputs(tag):
    plan = AU.plan_augmentation(META["cases"][tag]["augment"], DATA, _shard(tag))
    inp, out = GOLD[tag]["in"], GOLD[tag]["out"]
    got = A.apply(inp["ir_spectra"].numpy(), plan.src, plan.op["IR"], plan.op_table, plan.weights)
    assert np.array_equal(got.astype(np.float32), out["ir_spectra"].numpy().astype(np.float32))
    if "hnmr_spectra" in inp:                                    # the column that is not augmented is duplicated
        assert np.array_equal(inp["hnmr_spectra"].numpy()[plan.src], out["hnmr_spectra"].numpy().astype(np.float32))


def test_gaussian_weights_are_normalised_and_symmetric():
    for sigma in (0.3, 0.75, 1.25, 2.0, 12.0):
        r, w = AU.gaussian_half_kernel(sigma)
        assert r == int(4.0 * sigma + 0.5) and w.size == r + 1
        assert abs(w[0] + 2 * w[1:].sum() - 1.0) < 1e-12 and (np.diff(w) < 0).all()


def test_train_steps_count_the_expanded_set():
    n = 40
    cfg = _cfg("augment=ir/horizontal", "model.batch_size=8", "trainer.acc_batches=2", "trainer.epochs=3")
    train = {"meta": {"Formula": {"vocab_size": 16}, "Smiles": {"vocab_size": 16}},
             "data": {"IR": {"spectra": torch.rand(n, 1791)}}}
    aug = AU.plan_augmentation(cfg["augment"], cfg["data"], train)
    assert aug.rows == 3 * n
    plan = T.build_plan(cfg, train["meta"], aug.rows)
    assert plan["train_steps"] == calculate_training_steps(3 * n, 8, 2, 3) == 24
    assert plan["train_steps"] != T.build_plan(cfg, train["meta"], n)["train_steps"]


def test_refusals():
    train = {"meta": {}, "data": {"IR": {"spectra": torch.rand(3, 1791)}}}
    dc = _cfg()["data"]
    for name in ("combined", "smiles"):
        with pytest.raises(NotImplementedError, match="RDKit"):
            AU.plan_augmentation(_cfg(f"augment=ir/{name}")["augment"], dc, train)
        with pytest.raises(NotImplementedError, match="RDKit"):      # before the placeholder path of combined.yaml is read
            T.augment_train(_cfg(f"augment=ir/{name}"), train, "cpu")
    text = {"augment_data_path": None, "augmentations": [{"augment_column": "smiles", "augment_fns": {"horizontal": {"n_augments": 2}}}]}
    with pytest.raises(NotImplementedError, match="1D_patches"):
        AU.plan_augmentation(text, dc, train)
    unknown = {"augment_data_path": None, "augmentations": [{"augment_column": "raman", "augment_fns": {"smooth": {"sigmas": [1.0]}}}]}
    with pytest.raises(KeyError, match="raman"):
        AU.plan_augmentation(unknown, dc, train)
    # L % n == 0: the reference raises ValueError (interp1d's length check) -- so does the planner
    assert META["error_1800_n2"]["type"] == "ValueError"
    flat = {"meta": {}, "data": {"IR": {"spectra": torch.rand(3, 1800)}}}
    with pytest.raises(ValueError, match="n_augments=2"):
        AU.plan_augmentation(_cfg("augment=ir/horizontal")["augment"], dc, flat)
    hole = {"meta": {}, "data": {"IR": {"spectra": torch.rand(3, 1791), "present": torch.tensor([1, 0, 1], dtype=torch.bool)}}}
    with pytest.raises(ValueError, match="present == 0"):
        AU.plan_augmentation(_cfg("augment=ir/smooth")["augment"], dc, hole)
    # augment_data_path: a missing directory, the placeholder included
    with pytest.raises(FileNotFoundError):
        T.augment_train(_cfg("augment=ir/pseudo"), train, "cpu")
    with pytest.raises(FileNotFoundError):
        AU.load_extra("/nonexistent/augment", {})
    # on the fly with a mixture group: refused, not silently materialised
    with pytest.raises(NotImplementedError, match="mixture"):
        T.augment_train(_cfg("augment=ir/smooth", "+augment.on_the_fly=true"), train, "cpu", mixture={"balanced": {}})


def test_extra_rows_are_appended_after_the_blocks(tmp_path):
    train = {"meta": {"Smiles": {"vocab_size": 16, "pad_token_id": 0}},
             "data": {"IR": {"spectra": torch.rand(4, 1791)}, "Smiles": {"input_ids": torch.zeros(4, 5, dtype=torch.long)}}}
    extra = {"meta": {"Smiles": {"vocab_size": 16, "pad_token_id": 0}},
             "data": {"IR": {"spectra": torch.rand(2, 1791)}, "Smiles": {"input_ids": torch.ones(2, 5, dtype=torch.long)}}}
    torch.save(extra, os.path.join(str(tmp_path), "train.pt"))
    cfg = _cfg("augment=ir/smooth", f"augment.augment_data_path={tmp_path}")
    got = AU.load_extra(cfg["augment"]["augment_data_path"], train["meta"])
    plan = AU.plan_augmentation(cfg["augment"], cfg["data"], train, n_extra=AU.shard_rows(got))
    assert plan.rows == 4 + 8 + 2 and list(plan.src[-2:]) == [4, 5] and not plan.op["IR"][-2:].any()
    base = AU.base_data(train, got)
    assert base["IR"]["spectra"].shape == (6, 1791) and base["Smiles"]["input_ids"][4:].eq(1).all()
    with pytest.raises(ValueError, match="meta"):
        AU.load_extra(str(tmp_path), {"Smiles": {"vocab_size": 32, "pad_token_id": 0}})
