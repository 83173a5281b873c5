"""GPU: deterministic mode.  Each atomic-free export -- weight gradients (MFMA slab and fp32 FMA kernels, with and without the gated
FFN's interleave), column sums, LayerNorm dgamma / dbeta (vectorised and scalar kernels, every dy dtype), the cross-entropy loss
sum, the masked-mean pooling and the alignment loss (every kind) -- against an fp64 torch reference and against itself over three
repeats (torch.equal); the embedding scatter-add bit-exact against a CPU emulation of its stated order; whole training steps -- every
precision mode, the alignment head, the gated FFN, packed multi-modality batches, a checkpoint resume -- bit-identical between two
fresh runs; and one optimiser step agreeing with the default mode in the parameters and both Adam moments.  The default path's
run-to-run differences on the same shapes are recorded (record_parity), not asserted: they show what the tests would catch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import golden_io as G  # noqa: E402
from tests.conftest import record_parity  # noqa: E402

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------ weight gradients
def _operand(x, kind):
    from multimodalanalytical_amd.x2 import X2
    return X2.from_float(x) if kind == "x2" else x.to(kind)


def _value(x, kind):
    return x.float()


WGRAD_CASES = [
    # (M, N, K, operand dtype, glu_rows, packed live rows)
    (512, 512, 131072, torch.float16, 0, True),        # c2 wgrad group members, padded rows packed to the front (k_live + deal)
    (1536, 512, 131072, torch.bfloat16, 0, True),
    (2048, 512, 16384, torch.float16, 1024, False),    # gated FFN up-projection (glu_rows): rows of C / a_colsum de-interleaved
    (512, 2048, 16384, torch.bfloat16, 0, False),
    (128, 512, 16384, torch.float16, 0, False),        # the LM head's gradient: below the grouped kernel's shapes (generic det kernel)
    (512, 384, 8192, torch.float32, 0, False),         # fp32 mode
    (256, 256, 4096, "x2", 0, False),                  # split pairs (bf16x3)
    (512, 384, 8192, torch.float32, 256, False),       # the fp32 FMA det kernel with the gated FFN's interleave
    (256, 256, 4096, "x2", 128, False),                # ... and on split pairs
    (40, 8, 9000, torch.float32, 0, False),            # skinny and ragged
]


def _wgrad_problem(M, N, K, kind, live, seed):
    from multimodalanalytical_amd import ops
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(K, M, generator=g) * 0.5
    b = torch.randn(K, N, generator=g) * 0.5
    hint = None
    if live:
        nlive = (K // 64) * 5 // 8
        a[nlive * 64:] = 0
        t = torch.zeros(K // 64, dtype=torch.uint8)
        t[:nlive] = 1
        hint = ops.RowFlags(t.to(DEV), dealt=True)
    A, B = _operand(a.to(DEV), kind), _operand(b.to(DEV), kind)
    return A, B, hint


def _run_wgrad(A, B, M, N, glu_rows, hint, det):
    from multimodalanalytical_amd import ops
    C = torch.full((M, N), 0.25, device=DEV)
    cs = torch.full((M,), -0.5, device=DEV)
    kw = dict(trans_a=True, trans_b=False, accumulate=True, a_colsum=cs, glu_rows=glu_rows)
    if hint is not None:
        kw["k_live"] = hint
    if det:
        with ops.deterministic(ops.DetWorkspace(DEV)):
            ops.gemm_group([ops.gemm_desc(A, B, C, **kw)])
    else:
        ops.gemm_group([ops.gemm_desc(A, B, C, **kw)])
    torch.cuda.synchronize()
    return C, cs


def _deint(f, M):
    """Row of C that row m of the interleaved operand holds (afm_cast_weights glu_rows)."""
    m = torch.arange(M)
    return ((m >> 3) << 2) + (m & 3) + ((m >> 2) & 1) * f


@pytest.mark.parametrize("M,N,K,kind,glu_rows,live", WGRAD_CASES)
def test_wgrad_det_matches_fp64_and_repeats_bit_for_bit(M, N, K, kind, glu_rows, live):
    _need_gpu()
    A, B, hint = _wgrad_problem(M, N, K, kind, live, seed=M * 7 + N + K)
    a64, b64 = _value(A, kind).double(), _value(B, kind).double()
    ref = a64.t() @ b64 + 0.25
    ref_cs = a64.sum(0) - 0.5
    if glu_rows:
        r = _deint(glu_rows, M).to(DEV)
        ref = torch.empty_like(ref).index_copy_(0, r, ref)
        ref_cs = torch.empty_like(ref_cs).index_copy_(0, r, ref_cs)
    runs = [_run_wgrad(A, B, M, N, glu_rows, hint, det=True) for _ in range(3)]
    C, cs = runs[0]
    scale = float(ref.abs().max())
    err = float((C.double() - ref).abs().max()) / scale
    assert err < 2e-5, err
    assert float((cs.double() - ref_cs).abs().max()) / float(ref_cs.abs().max()) < 1e-4
    for C2, cs2 in runs[1:]:
        assert torch.equal(C, C2) and torch.equal(cs, cs2)
    # the default path on the same problem: how many elements move between repeats (a record, not an assertion)
    from multimodalanalytical_amd import lib as L
    try:
        dflt = [_run_wgrad(A, B, M, N, glu_rows, hint, det=False) for _ in range(3)]
        moved = sum(int((d[0] != dflt[0][0]).sum()) + int((d[1] != dflt[0][1]).sum()) for d in dflt[1:])
    except L.AfmError:          # (the default kernels have no interleaved fp32 wgrad: the engine does not ask for one)
        moved = None
    record_parity("test_wgrad_det_matches_fp64_and_repeats_bit_for_bit", shape=[M, N, K], dtype=str(kind), glu_rows=glu_rows,
                  det_rel_err=err, default_elements_changed_over_3_repeats=moved)


def test_wgrad_det_group_of_a_c2_layer_repeats_and_matches_fp64():
    """One call over a layer's four weight gradients (one grouped launch, one shared chunk length): fp64 agreement and equal bits
    over repeats, with fresh workspaces and a reused one."""
    _need_gpu()
    from multimodalanalytical_amd import ops
    probs = [(1536, 512), (512, 512), (2048, 512), (512, 2048)]
    K = 32768
    ins = [_wgrad_problem(M, N, K, torch.float16, True, seed=M + N) for M, N in probs]
    ws = ops.DetWorkspace(DEV)

    def run(w):
        outs, descs = [], []
        for (M, N), (A, B, hint) in zip(probs, ins):
            C, cs = torch.zeros(M, N, device=DEV), torch.zeros(M, device=DEV)
            outs.append((C, cs))
            descs.append(ops.gemm_desc(A, B, C, trans_a=True, trans_b=False, accumulate=True, a_colsum=cs, k_live=hint))
        ops.gemm_group_det(descs, w)
        torch.cuda.synchronize()
        return outs
    first = run(ws)
    for again in (run(ws), run(ops.DetWorkspace(DEV))):
        for x, y in zip(first, again):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    for (C, cs), (A, B, _) in zip(first, ins):
        ref = A.double().t() @ B.double()
        assert float((C.double() - ref).abs().max()) / float(ref.abs().max()) < 2e-5
        torch.testing.assert_close(cs.double(), A.double().sum(0), rtol=1e-4, atol=1e-4 * float(A.double().sum(0).abs().max()))


def test_det_gemm_refuses_what_it_cannot_honour():
    _need_gpu()
    from multimodalanalytical_amd import lib as L, ops
    a = torch.randn(4096, 256, device=DEV, dtype=torch.float16)
    b = torch.randn(4096, 256, device=DEV, dtype=torch.float16)
    C = torch.zeros(256, 256, device=DEV)
    d = ops.gemm_desc(a, b, C, trans_a=True, trans_b=False, accumulate=True)
    arr = (L.GemmDesc * 1)(d)
    h = L.load()
    ptr = __import__("ctypes").cast(arr, __import__("ctypes").c_void_p)
    need = h.afm_gemm_group_det_ws_floats(ptr, 1)
    small = torch.empty(max(need // 2, 4), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert need > 0 and h.afm_gemm_group_det(ptr, 1, None, 0, s) == -1
    assert h.afm_gemm_group_det(ptr, 1, small.data_ptr(), small.numel(), s) == -1
    arr[0].reserved2 |= 16                      # the deterministic bit: afm_gemm / afm_gemm_group have no workspace for the wgrad form
    assert h.afm_gemm(__import__("ctypes").byref(arr[0]), s) == -2
    assert h.afm_gemm_group(ptr, 1, s) == -2
    e = ops.gemm_desc(a, b, torch.zeros(4096, 4096, device=DEV), trans_a=False, trans_b=True)      # not a weight gradient
    arr2 = (L.GemmDesc * 1)(e)
    ws = torch.empty(1 << 20, device=DEV)
    assert h.afm_gemm_group_det(__import__("ctypes").cast(arr2, __import__("ctypes").c_void_p), 1, ws.data_ptr(), ws.numel(), s) == -2
    torch.cuda.synchronize()
    assert float(C.abs().max()) == 0.0          # nothing was launched


# ------------------------------------------------------------------------------------------------ other reductions
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_colsum_det(dtype):
    _need_gpu()
    from multimodalanalytical_amd import ops
    x = (torch.randn(70001, 300, device=DEV) * 3).to(dtype)
    ref = x.double().sum(0)
    outs = []
    for _ in range(3):
        out = torch.full((300,), 1.0, device=DEV)
        ops.colsum_det(x, out, accumulate=True, ws=ops.DetWorkspace(DEV))
        outs.append(out)
    assert float((outs[0].double() - 1.0 - ref).abs().max()) < 1e-5 * float(x.double().abs().sum(0).max())
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    out = torch.full((300,), 7.0, device=DEV)
    ops.colsum_det(x, out, accumulate=False)
    torch.testing.assert_close(out, outs[0] - 1.0, rtol=1e-6, atol=1e-4)


def _scatter_cpu(ids, dout, table, scale, pad):
    """Sequential fp32 emulation of afm_scatter_add_rows_det: rows in ascending order, product and sum rounded one at a time."""
    import numpy as np
    t = table.cpu().numpy().copy()
    d = dout.cpu().numpy()
    s = None if scale is None else scale.cpu().numpy()
    V = t.shape[0]
    for r, i in enumerate(ids.cpu().tolist()):
        if i == pad:
            continue
        v = min(max(i, 0), V - 1)
        term = d[r] if s is None else (d[r] * np.float32(s[r])).astype(np.float32)
        t[v] = (t[v] + term).astype(np.float32)
    return torch.from_numpy(t)


@pytest.mark.parametrize("with_scale", [False, True])
def test_scatter_add_rows_det_is_bit_exact_vs_sequential_cpu_sum(with_scale):
    _need_gpu()
    from multimodalanalytical_amd import ops
    g = torch.Generator().manual_seed(5)
    V, d, n, pad = 37, 200, 5000, 0
    ids = torch.randint(0, V, (n,), generator=g)
    ids[::7] = pad                                  # padding rows
    ids[100:400] = 3                                # one row repeated many times
    ids[10], ids[11] = -4, V + 9                    # out of range: clamped
    dout = torch.randn(n, d, generator=g)
    scale = torch.rand(n, generator=g) + 0.5 if with_scale else None
    table = torch.randn(V, d, generator=g)
    ref = _scatter_cpu(ids, dout, table, scale, pad)
    for _ in range(3):
        t = table.to(DEV)
        ops.scatter_add_rows_det(ids.to(DEV), dout.to(DEV), t, None if scale is None else scale.to(DEV), padding_idx=pad)
        assert torch.equal(t.cpu(), ref)
    t = table.to(DEV)
    with ops.deterministic(ops.DetWorkspace(DEV)):             # the routed form is the same call
        ops.scatter_add_rows(ids.to(DEV), dout.to(DEV), t, None if scale is None else scale.to(DEV), padding_idx=pad)
    assert torch.equal(t.cpu(), ref)


# ------------------------------------------------------------------------------------------------ whole training steps
MODES = ["fp16", "bf16", "fp32", "bf16x3-mixed", "bf16x3"]


def _dtypes(mode):
    from multimodalanalytical_amd.x2 import X2
    return {"fp16": (torch.float16, None), "bf16": (torch.bfloat16, None), "fp32": (torch.float32, None),
            "bf16x3-mixed": (X2.dtype, torch.bfloat16), "bf16x3": (X2.dtype, None)}[mode]


def _wrapper(t, mode, deterministic):
    _need_gpu()
    from multimodalanalytical_amd.modeling.wrapper import HFWrapper, SimpleTokenizerInfo
    m = t["meta"]
    cfg = G.model_cfg(m)
    mk = {k: v for k, v in cfg.items() if k != "multimodal_norm"}
    cd, bd = _dtypes(mode)
    kw = {"backward_dtype": bd} if bd is not None else {}
    w = HFWrapper(m["data_config"], "CustomModel", "facebook/bart-base", SimpleTokenizerInfo(26), optimiser=m["optimiser"],
                  lr=mk.pop("lr", m["lr"]), weight_decay=m["weight_decay"], num_steps=m["total_steps"], device=DEV, compute_dtype=cd,
                  deterministic=deterministic, **kw, **mk)
    w.hf_model.load_state_dict(t["sd"])
    return w


def _dev_batch(t, i):
    from multimodalanalytical_amd.synth import to_device
    return to_device(G.batch_of(t, i), DEV)


def _train(t, mode, deterministic, n=6, loop_state=None):
    from multimodalanalytical_amd.trainer import TrainLoop
    w = _wrapper(t, mode, deterministic)
    loop = TrainLoop(w, acc_batches=2)
    losses = torch.stack([loop.micro_batch(_dev_batch(t, i % 4)).detach().clone() for i in range(n)])
    torch.cuda.synchronize()
    return w, loop, losses


def _state(w):
    e = w.hf_model.engine
    return {"flat": e.ps.flat, "exp_avg": e.ps.exp_avg, "exp_avg_sq": e.ps.exp_avg_sq,
            "scaler": e.scaler if e.scaler is not None else torch.zeros(1, device=DEV)}


def _assert_same_run(a, b, la, lb):
    assert torch.equal(la, lb), (la, lb)
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (k, float((sa[k] - sb[k]).abs().max()), int((sa[k] != sb[k]).sum()))


@pytest.mark.parametrize("mode", MODES)
def test_training_steps_are_bit_identical(mode):
    t = G.load("model_plain")
    a, _, la = _train(t, mode, True)
    assert a.hf_model.engine.deterministic
    b, _, lb = _train(t, mode, True)
    _assert_same_run(a, b, la, lb)
    # the default mode on the same run: how many parameters part (a record)
    c, _, lc = _train(t, mode, False)
    d, _, ld = _train(t, mode, False)
    record_parity("test_training_steps_are_bit_identical", mode=mode, golden="model_plain",
                  default_params_changed=int((_state(c)["flat"] != _state(d)["flat"]).sum()),
                  default_losses_equal=bool(torch.equal(lc, ld)))


@pytest.mark.parametrize("name,mode", [("model_align_mlp_mse", "fp16"), ("model_align_conv_sid", "fp32"),
                                       ("model_gated_learned", "bf16"), ("model_postln_gated", "fp16")])
def test_training_steps_are_bit_identical_with_alignment_head_and_gated_ffn(name, mode):
    t = G.load(name)
    a, _, la = _train(t, mode, True)
    b, _, lb = _train(t, mode, True)
    _assert_same_run(a, b, la, lb)


def test_training_steps_are_bit_identical_on_packed_multimodal_batches():
    """The c3 workload (text + IR patches + ...; padded samples, rows packed to the front by default: AFM_FWD_COMPACT=2) at a small
    batch: 4 micro-batches at acc_batches = 2, twice from the same seed."""
    _need_gpu()
    from multimodalanalytical_amd import synth
    from multimodalanalytical_amd.modeling.wrapper import HFWrapper, SimpleTokenizerInfo
    from multimodalanalytical_amd.trainer import TrainLoop
    wl = synth.WORKLOADS["c3"]
    batches = [synth.make_batch("c3", 8, seed=60 + i, device=DEV)[0] for i in range(4)]

    def run():
        w = HFWrapper(wl["data"], "CustomModel", "facebook/bart-base", SimpleTokenizerInfo(wl["data"]["Smiles"]["vocab_size"]),
                      optimiser="adamw", lr=1e-4, num_steps=10, device=DEV, compute_dtype=torch.float16, seed=5, deterministic=True,
                      **{k: v for k, v in wl["cfg"].items() if k != "multimodal_norm"})
        loop = TrainLoop(w, acc_batches=2)
        ls = torch.stack([loop.micro_batch(b).detach().clone() for b in batches])
        torch.cuda.synchronize()
        return w, ls
    a, la = run()
    b, lb = run()
    assert a.hf_model.engine.fwd_compact == 2
    _assert_same_run(a, b, la, lb)


def test_fp16_checkpoint_resume_is_exact_in_deterministic_mode(tmp_path):
    """The resume scenario of test_gpu_model.py::test_fp16_checkpoint_resume_continues_the_run with no masks and no tolerances."""
    from multimodalanalytical_amd.trainer import TrainLoop, load_checkpoint, save_checkpoint
    t = G.load("model_plain")

    def fresh():
        w = _wrapper(t, "fp16", True)
        return w, TrainLoop(w, acc_batches=2)
    w, loop = fresh()
    for i in range(6):
        loop.micro_batch(_dev_batch(t, i % 4))
    path = str(tmp_path / "det.ckpt")
    save_checkpoint(path, w, loop, epoch=1)
    w2, loop2 = fresh()
    load_checkpoint(path, w2, loop2)
    la, lb = [], []
    for i in range(6, 10):
        la.append(loop.micro_batch(_dev_batch(t, i % 4)).detach().clone())
        lb.append(loop2.micro_batch(_dev_batch(t, i % 4)).detach().clone())
    torch.cuda.synchronize()
    _assert_same_run(w, w2, torch.stack(la), torch.stack(lb))
    assert loop.optim.step_count == loop2.optim.step_count == 5


@pytest.mark.parametrize("name,mode", [("model_plain", "fp32"), ("model_align_conv_sid", "fp32"), ("model_align_mlp_mse", "fp16"),
                                       ("model_gated_learned", "bf16")])
def test_deterministic_mode_computes_the_same_math(name, mode):
    """One optimiser step, det against default: the losses, the parameters that have a gradient, and both Adam moments -- exp_avg is
    0.1 g and exp_avg_sq 0.001 g^2 after one step, so a gradient scaled or missing a share of its partial sums shows there even where
    Adam's first update (about lr * sign(g)) would not."""
    t = G.load(name)
    a, _, la = _train(t, mode, True, n=2)
    b, _, lb = _train(t, mode, False, n=2)
    tol = 2e-5 if mode == "fp32" else 2e-4
    torch.testing.assert_close(la, lb, rtol=tol, atol=tol)
    sa, sb = _state(a), _state(b)
    has_grad = sb["exp_avg_sq"] > max(1e-14, 1e-10 * float(sb["exp_avg_sq"].max()))
    assert float(has_grad.float().mean()) > 0.9
    d = float((sa["flat"] - sb["flat"])[has_grad].abs().max())
    assert d < 2e-5, d
    for k, rtol in (("exp_avg", 20 * tol), ("exp_avg_sq", 40 * tol)):
        big = float(sb[k].abs().max())
        torch.testing.assert_close(sa[k], sb[k], rtol=rtol, atol=1e-4 * big, msg=lambda m: f"{k}: {m}")
    assert torch.equal(sa["scaler"], sb["scaler"])


# ------------------------------------------------------------------------------------------------ LayerNorm, loss, alignment head
def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _dy(x, kind):
    from multimodalanalytical_amd.x2 import X2
    return X2.from_float(x.to(DEV)) if kind == "x2" else x.to(DEV).to(kind)


@pytest.mark.parametrize("kind", [torch.float32, torch.bfloat16, torch.float16, "x2"])
@pytest.mark.parametrize("rows,d", [(4096, 512), (1000, 768), (150, 36)])      # vectorised kernel (d % 8 == 0, rows >= 64); scalar kernel
def test_layernorm_bwd_det_matches_fp64_and_repeats(kind, rows, d):
    _need_gpu()
    from multimodalanalytical_amd import ops
    from oracle import afm_oracle as O
    x = _rnd(rows, d, seed=1) * 2 + 0.5
    gam, bet = 1 + 0.1 * _rnd(d, seed=2), 0.1 * _rnd(d, seed=3)
    y = torch.empty(rows, d, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    ops.layernorm_fwd(x.to(DEV), gam.to(DEV), bet.to(DEV), y, mean, rstd)
    dy = _dy(_rnd(rows, d, seed=5), kind)
    dres = _rnd(rows, d, seed=6).to(DEV)
    xr, gr, br = (v.double().requires_grad_(True) for v in (x, gam, bet))
    O.layer_norm(xr, gr, br).backward(dy.float().cpu().double())
    dg0, db0 = _rnd(d, seed=7), _rnd(d, seed=8)
    outs = []
    for _ in range(3):
        dx = torch.empty(rows, d, device=DEV)
        dg, db = dg0.to(DEV), db0.to(DEV)
        with ops.deterministic(ops.DetWorkspace(DEV)):
            ops.layernorm_bwd(dy, x.to(DEV), gam.to(DEV), mean, rstd, dx, dg, db, torch.empty(0, device=DEV), dres=dres)
        torch.cuda.synchronize()
        outs.append((dx, dg, db))
    dx, dg, db = outs[0]
    for o in outs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(outs[0], o))
    torch.testing.assert_close(dx.cpu().double(), xr.grad + dres.cpu().double(), rtol=1e-4, atol=1e-5)
    for got, base, ref in ((dg, dg0, gr.grad), (db, db0, br.grad)):
        want = base.double() + ref
        torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=1e-5 * float(want.abs().max()))
    # and the default kernels on the same call, within their own tolerance
    dx2, dg2, db2 = torch.empty(rows, d, device=DEV), dg0.to(DEV), db0.to(DEV)
    ops.layernorm_bwd(dy, x.to(DEV), gam.to(DEV), mean, rstd, dx2, dg2, db2,
                      torch.empty(ops.layernorm_bwd_ws(rows, d), device=DEV), dres=dres)
    assert torch.equal(dx2, dx)              # (dx takes no cross-block sum: the same bits either way)
    torch.testing.assert_close(dg2, dg, rtol=1e-5, atol=1e-5 * float(dg.abs().max()))
    torch.testing.assert_close(db2, db, rtol=1e-5, atol=1e-5 * float(db.abs().max()))


def test_ce_fwd_det_matches_fp64_and_repeats():
    _need_gpu()
    from multimodalanalytical_amd import ops
    rows, V = 16383, 61                      # (not a multiple of the 4 rows a block takes)
    logits = _rnd(rows, V, seed=1) * 3
    labels = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(2))
    labels[::5] = -100
    lse64 = torch.logsumexp(logits.double(), 1)
    keep = labels != -100
    ref_loss = float((lse64[keep] - logits.double()[keep, labels[keep]]).sum())
    outs = []
    for det in (True, True, True, False):
        stats = torch.tensor([0.5, 2.0], device=DEV)
        lse, am = torch.empty(rows, device=DEV), torch.empty(rows, dtype=torch.int64, device=DEV)
        if det:
            with ops.deterministic(ops.DetWorkspace(DEV)):
                ops.ce_fwd(logits.to(DEV), labels.to(DEV), lse, am, stats)
        else:
            ops.ce_fwd(logits.to(DEV), labels.to(DEV), lse, am, stats)
        torch.cuda.synchronize()
        outs.append((stats, lse, am))
    stats, lse, am = outs[0]
    for o in outs[1:3]:
        assert all(torch.equal(u, v) for u, v in zip(outs[0], o))
    assert float(stats[1]) == 2.0 + int(keep.sum())
    assert abs(float(stats[0]) - 0.5 - ref_loss) < 1e-5 * abs(ref_loss)
    torch.testing.assert_close(lse.cpu().double(), lse64, rtol=1e-5, atol=1e-5)
    assert torch.equal(lse, outs[3][1]) and torch.equal(am, outs[3][2])       # per-row outputs: the default kernel's bits
    assert abs(float(outs[3][0][0]) - float(stats[0])) < 1e-5 * abs(ref_loss) and float(outs[3][0][1]) == float(stats[1])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,S,d", [(5, 777, 96), (64, 1024, 512)])
def test_masked_mean_fwd_det_matches_fp64_and_repeats(dt, B, S, d):
    _need_gpu()
    from multimodalanalytical_amd import ops
    x = _rnd(B * S, d, seed=1).to(dt)
    pad = torch.rand(B, S, generator=torch.Generator().manual_seed(2)) < 0.4
    pad[:, 0] = False
    keep = (~pad).double().unsqueeze(-1)
    ref = (x.double().view(B, S, d) * keep).sum(1) / keep.sum(1)
    outs = []
    for _ in range(3):
        out = torch.full((B, d), 9.0, device=DEV)
        with ops.deterministic(ops.DetWorkspace(DEV)):
            ops.masked_mean_fwd(x.to(DEV), pad.to(torch.uint8).to(DEV), B, S, out)
        torch.cuda.synchronize()
        outs.append(out)
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    torch.testing.assert_close(outs[0].cpu().double(), ref, rtol=1e-5, atol=1e-6)
    dflt = torch.empty(B, d, device=DEV)
    ops.masked_mean_fwd(x.to(DEV), pad.to(torch.uint8).to(DEV), B, S, dflt)
    torch.testing.assert_close(dflt, outs[0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kind", ["mse", "mae", "sid"])
def test_align_loss_det_matches_fp64_and_repeats(kind):
    _need_gpu()
    from multimodalanalytical_amd import ops
    B, n = 128, 1800                         # 900 blocks of partial sums
    z = _rnd(B, n, seed=1)
    tgt = torch.rand(B, n, generator=torch.Generator().manual_seed(2))
    tgt[:, ::7] = 0.0
    p = torch.sigmoid(z.double())
    if kind == "mse":
        ref = float(((p - tgt.double()) ** 2).mean())
    elif kind == "mae":
        ref = float((p - tgt.double()).abs().mean())
    else:
        pc, tc = p.clamp(min=1e-16), tgt.double().clamp(min=1e-16)
        ref = float((pc * (pc / tc).log()).sum() / B + (tc * (tc / pc).log()).sum() / B)
    outs = []
    for det in (True, True, True, False):
        stats, dz = torch.tensor([0.25], device=DEV), torch.empty(B, n, device=DEV)
        if det:
            with ops.deterministic(ops.DetWorkspace(DEV)):
                ops.align_loss(z.to(DEV), tgt.to(DEV), kind, 0.5, stats, dz)
        else:
            ops.align_loss(z.to(DEV), tgt.to(DEV), kind, 0.5, stats, dz)
        torch.cuda.synchronize()
        outs.append((stats, dz))
    for o in outs[1:3]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
    assert abs(float(outs[0][0]) - 0.25 - ref) < 2e-5 * abs(ref) + 1e-7
    assert torch.equal(outs[0][1], outs[3][1])                                 # dz: the default kernel's bits
    assert abs(float(outs[3][0]) - float(outs[0][0])) < 2e-5 * abs(ref) + 1e-7
