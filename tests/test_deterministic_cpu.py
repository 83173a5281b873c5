"""CPU: the deterministic mode's C ABI (declared, exported, bound; ABI version unchanged), its host-only workspace queries, and the
switches that turn it on (AFM_DETERMINISTIC, +trainer.deterministic=true).  No compute calls."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DET_EXPORTS = ["afm_gemm_group_det_ws_floats", "afm_gemm_group_det", "afm_colsum_det_ws_floats", "afm_colsum_det",
               "afm_scatter_add_rows_det", "afm_ce_fwd_det_ws_floats", "afm_ce_fwd_det", "afm_masked_mean_fwd_det_ws_floats",
               "afm_masked_mean_fwd_det", "afm_align_loss_det_ws_floats", "afm_align_loss_det"]


def test_det_exports_are_declared_exported_and_bound():
    from multimodalanalytical_amd import lib as L
    header = open(os.path.join(ROOT, "include", "afm_hip.h")).read()
    handle = L.load()
    for name in DET_EXPORTS:
        assert f"{name}(" in header, name
        assert hasattr(handle, name), name
        assert name in L.exported_symbols(), name
    assert handle.afm_abi_version() == 6


def _wgrad_desc(M, N, K, dtype, colsum=True, glu_rows=0):
    from multimodalanalytical_amd import lib as L
    d = L.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.transA, d.transB = 1, 0
    d.lda, d.ldb, d.ldc = M, N, N
    d.a_dtype = d.b_dtype = dtype
    d.c_dtype = L.AFM_F32
    d.accumulate = 1
    d.glu_rows = glu_rows
    if colsum:
        d.a_colsum = 4096        # (never dereferenced: the query looks at shapes only)
    return d


def _ws(descs):
    from multimodalanalytical_amd import lib as L
    arr = (L.GemmDesc * len(descs))(*descs)
    return int(L.load().afm_gemm_group_det_ws_floats(ctypes.cast(arr, ctypes.c_void_p), len(descs)))


def test_wgrad_workspace_query_is_host_only_and_depends_on_shapes_only():
    from multimodalanalytical_amd import lib as L
    K = 131072
    for dt in (L.AFM_F16, L.AFM_BF16, L.AFM_F32, L.AFM_BF16X2):
        enc = [_wgrad_desc(1536, 512, K, dt), _wgrad_desc(512, 512, K, dt), _wgrad_desc(2048, 512, K, dt), _wgrad_desc(512, 2048, K, dt)]
        if dt == L.AFM_BF16X2:
            for d in enc:
                d.lda, d.ldb = 2 * d.M, 2 * d.N
        n = _ws(enc)
        assert n > 0
        assert n == _ws(enc) and n == _ws([enc[0], enc[1], enc[2], enc[3]])        # repeatable: the plan is the shapes'
        # at most 16 (MFMA) / 64 (fp32 kernel, <= 2^24 floats) slabs of each dW plus the column-sum partials
        floats = sum(d.M * d.N for d in enc)
        slabs = 16 if dt in (L.AFM_F16, L.AFM_BF16) else 64
        assert floats <= n <= slabs * floats + slabs * 4 * 8 * sum(d.M for d in enc) + 16 * len(enc)
    # the pointers and the caller's accumulate / variant do not enter the plan
    a, b = _wgrad_desc(2048, 512, K, L.AFM_F16), _wgrad_desc(2048, 512, K, L.AFM_F16)
    b.A, b.B, b.C, b.accumulate, b.reserved = 1 << 20, 2 << 20, 3 << 20, 0, 105
    assert _ws([a]) == _ws([b])
    # gated FFN (c4: f = 3072 rows per half, d = 768) and a wgrad without a bias
    assert _ws([_wgrad_desc(6144, 768, 16384, L.AFM_BF16, glu_rows=3072)]) > 6144 * 768
    assert _ws([_wgrad_desc(512, 512, K, L.AFM_F16, colsum=False)]) < _ws([_wgrad_desc(512, 512, K, L.AFM_F16)])
    # not the weight-gradient form: refused (-1), never planned
    bad = _wgrad_desc(512, 512, K, L.AFM_F16)
    bad.transA = 0
    assert _ws([bad]) == -1
    bad = _wgrad_desc(512, 512, K, L.AFM_F16)
    bad.act = L.ACT_GELU
    assert _ws([bad]) == -1


def test_other_workspace_queries_are_host_only():
    from multimodalanalytical_amd import lib as L, ops
    h = L.load()
    assert h.afm_colsum_det_ws_floats(131072, 512) == 256 * 512
    assert h.afm_colsum_det_ws_floats(100, 64) == 64
    assert h.afm_ce_fwd_det_ws_floats(16384) == 2 * 4096
    assert h.afm_masked_mean_fwd_det_ws_floats(2, 1024, 512) > 0
    assert h.afm_align_loss_det_ws_floats(128, 300) > 0
    assert h.afm_colsum_det_ws_floats(10, 0) == -1
    # LayerNorm: the deterministic size (flags bit 1) exists for every shape, the default one is 0 where the kernel uses atomics
    assert ops.layernorm_bwd_ws(131072, 512) == 0
    assert ops.layernorm_bwd_ws(131072, 512, det=True) == 768 * 2 * 512
    assert ops.layernorm_bwd_ws(100, 36, det=True) > 0


def test_afm_deterministic_env_is_parsed_like_the_other_switches(monkeypatch):
    from multimodalanalytical_amd.engine import Seq2SeqEngine
    from tests import golden_io as G
    t = G.load("model_plain")
    cfg = G.model_cfg(t["meta"])
    vocab = t["meta"]["data_config"]["Smiles"]["vocab_size"]

    def build(**kw):
        return Seq2SeqEngine(cfg, t["meta"]["data_config"], "Smiles", vocab, device="cpu", compute_dtype=__import__("torch").float32, **kw)
    monkeypatch.delenv("AFM_DETERMINISTIC", raising=False)
    assert build().deterministic is False
    monkeypatch.setenv("AFM_DETERMINISTIC", "1")
    assert build().deterministic is True
    assert build(deterministic=False).deterministic is False       # an explicit argument wins
    monkeypatch.setenv("AFM_DETERMINISTIC", "0")
    assert build().deterministic is False
    assert build(deterministic=True).deterministic is True


def test_cli_accepts_trainer_deterministic_and_passes_it_to_the_model(monkeypatch):
    from multimodalanalytical_amd import config as CFG
    from multimodalanalytical_amd.cli import training as T
    from multimodalanalytical_amd.synth import synth_shards
    cfg = CFG.compose(os.path.join(ROOT, "configs"), "config_train", ["model=custom_model", "+trainer.deterministic=true"])
    assert cfg["trainer"]["deterministic"] is True
    shards = synth_shards(cfg["data"], 16, 8, 8, seed=1)
    plan = T.build_plan(cfg, shards["train"]["meta"], 1000)
    assert plan["deterministic"] is True
    plain = CFG.compose(os.path.join(ROOT, "configs"), "config_train", ["model=custom_model"])
    assert T.build_plan(plain, shards["train"]["meta"], 1000)["deterministic"] is None      # unset: AFM_DETERMINISTIC decides
    # the flag reaches the engine through HFWrapper's keyword arguments
    seen = {}
    from multimodalanalytical_amd.modeling import custom_modeling as CM

    class Stop(Exception):
        pass

    def fake_engine(*a, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(CM, "Seq2SeqEngine", fake_engine)
    from multimodalanalytical_amd.modeling.wrapper import HFWrapper, SimpleTokenizerInfo
    dc = plan["data_config"]
    tm = plan["target_modality"]
    mk = {k: v for k, v in plan["model_config"].items() if k != "multimodal_norm"}
    with pytest.raises(Stop):
        HFWrapper(dc, target_tokenizer=SimpleTokenizerInfo(dc[tm]["vocab_size"]), device="cpu", deterministic=plan["deterministic"], **mk)
    assert seen["deterministic"] is True
