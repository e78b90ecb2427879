"""The decoder's one-key cross-attention fast path (fpnmt.config.cross_one_key).

With one unmasked encoder key the softmax weight is exactly 1, so a decoder
layer's cross-attention sublayer is LN2(out1 + dropout(v W_o + b_o)) with the
same Dense row for all T positions of an image. Checked here:

1. fpnmt_layernorm_bcast_fwd against fpnmt_layernorm_fwd on the materialised
   x, bit for bit (y, mean, rstd, and the x it optionally stores);
2. fpnmt_layernorm_bcast_bwd against fpnmt_layernorm_bwd_drop on that x, bit
   for bit (dx, dz, dgamma, dbeta), and fpnmt_rowsum_groups against an fp64 sum;
3. a Decoder with the switch on against the switch off (fp32: 1e-5 of each
   tensor's max; bf16: error against the fp32 general path at most 25 % above
   the general bf16 path's; q / k gradients exactly zero);
4. routing (two keys, or a padding mask, take the general path: seen in the
   launch log of a child process, results bitwise equal on / off);
5. a TrainEngine step: graph replay equals eager, two runs equal, bit for bit.
"""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(3, 5, 192), (2, 31, 512), (2, 3, 100)]  # (B, T, d); 100: not a multiple of 8 (scalar path)
SEED, STEP = 0x1234567, 7


def _lib():
    from fpnmt import _lib as L
    return L, L.call, L.ptr, L.stream_ptr, L.dtype_code


def _case(B, T, d, dtype, p):
    """Inputs of one LayerNorm case and the materialised x: the Dense output
    (c + bias) broadcast over T under fpnmt_dropout's mask for (SEED, STEP)."""
    L, call, ptr, sp, code = _lib()
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + d)
    c = torch.randn(B, d, generator=g).to(DEV)
    cb = torch.randn(d, generator=g).to(DEV)
    res = torch.randn(B, T, d, generator=g).to(DEV).to(dtype)
    gamma = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=g)).to(DEV)
    dy = torch.randn(B, T, d, generator=g).to(DEV).to(dtype)
    st = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    mask = torch.ones(B, T, d, device=DEV)
    if p > 0:
        ones = torch.ones(B, T, d, device=DEV)
        call("fpnmt_dropout", L.F32, ones.numel(), p, SEED, ptr(st), ptr(ones), ptr(mask), sp())
    x = (((c + cb)[:, None, :]).expand(B, T, d) * mask).to(dtype).contiguous()
    return c, cb, res, gamma, beta, dy, st, x


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_layernorm_bcast_fwd_bitwise(shape, dtype, p):
    L, call, ptr, sp, code = _lib()
    B, T, d = shape
    rows = B * T
    c, cb, res, gamma, beta, dy, st, x = _case(B, T, d, dtype, p)
    out = []
    for fast in (False, True):
        y = torch.empty_like(res)
        mean = torch.empty(rows, device=DEV)
        rstd = torch.empty(rows, device=DEV)
        if fast:
            xs = torch.full_like(x, float("nan"))
            call("fpnmt_layernorm_bcast_fwd", code(dtype), rows, d, T, 1e-6, ptr(c), ptr(cb), p, SEED, ptr(st),
                 ptr(res), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(xs), sp())
            y2, m2 = torch.empty_like(res), torch.empty(rows, device=DEV)  # and without the stored x
            call("fpnmt_layernorm_bcast_fwd", code(dtype), rows, d, T, 1e-6, ptr(c), ptr(cb), p, SEED, ptr(st),
                 ptr(res), ptr(gamma), ptr(beta), ptr(y2), ptr(m2), ptr(torch.empty(rows, device=DEV)), None, sp())
        else:
            call("fpnmt_layernorm_fwd", code(dtype), rows, d, 1e-6, ptr(x), ptr(res), ptr(gamma), ptr(beta), None, 0,
                 ptr(y), ptr(mean), ptr(rstd), sp())
        out.append((y, mean, rstd))
    torch.cuda.synchronize()
    if p > 0:
        assert 0 < int((x == 0).sum()) < x.numel() // 2  # the mask dropped something, not everything
    for a, b, name in zip(out[0], out[1], ("y", "mean", "rstd")):
        assert torch.equal(a, b), name
    assert torch.equal(xs, x) and torch.equal(y2, out[1][0]) and torch.equal(m2, out[1][1])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_layernorm_bcast_bwd_bitwise(shape, dtype, p):
    L, call, ptr, sp, code = _lib()
    B, T, d = shape
    rows = B * T
    c, cb, res, gamma, beta, dy, st, x = _case(B, T, d, dtype, p)
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    y = torch.empty_like(res)
    call("fpnmt_layernorm_fwd", code(dtype), rows, d, 1e-6, ptr(x), ptr(res), ptr(gamma), ptr(beta), None, 0, ptr(y),
         ptr(mean), ptr(rstd), sp())
    out = []
    for fast in (False, True):
        dx = torch.empty_like(res)
        dz = torch.empty_like(res)
        dg = torch.zeros(d, device=DEV)
        db = torch.zeros(d, device=DEV)
        if fast:
            call("fpnmt_layernorm_bcast_bwd", code(dtype), rows, d, T, ptr(c), ptr(cb), p, SEED, ptr(st), ptr(res),
                 ptr(gamma), ptr(mean), ptr(rstd), ptr(dy), ptr(dx), ptr(dg), ptr(db), ptr(dz) if p > 0 else None,
                 sp())
        elif p > 0:
            call("fpnmt_layernorm_bwd_drop", code(dtype), rows, d, ptr(x), ptr(res), ptr(gamma), ptr(mean), ptr(rstd),
                 ptr(dy), ptr(dx), ptr(dg), ptr(db), p, SEED, ptr(st), ptr(dz), sp())
        else:
            call("fpnmt_layernorm_bwd", code(dtype), rows, d, ptr(x), ptr(res), ptr(gamma), ptr(mean), ptr(rstd),
                 ptr(dy), ptr(dx), ptr(dg), ptr(db), sp())
        torch.cuda.synchronize()
        out.append((dx, dz if p > 0 else dx, dg, db))  # p == 0: the Dense's gradient is dx itself
    for a, b, name in zip(out[0], out[1], ("dx", "dz", "dgamma", "dbeta")):
        assert torch.equal(a, b), name
    assert float(out[1][2].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_rowsum_groups(shape, dtype):
    """dc within T * 2^-24 * sum|dz| of the fp64 sum (T fp32 additions, each
    within 2^-24 relative of a partial sum that is at most sum|dz|), two runs
    bitwise equal, the rounded copy and the zeroed key-gradient blocks."""
    L, call, ptr, sp, code = _lib()
    B, T, d = shape
    n = 3
    g = torch.Generator().manual_seed(5)
    dzs = [torch.randn(B * T, d, generator=g).to(DEV).to(dtype) for _ in range(n)]
    tab = (ctypes.c_void_p * n)(*[z.data_ptr() for z in dzs])
    runs = []
    for _ in range(2):
        dc = torch.full((n, B, d), float("nan"), device=DEV)
        lp = torch.full((n, B, d), float("nan"), device=DEV).to(dtype)
        buf = torch.full((B, 2 * n * d + 8), 3.0, device=DEV).to(dtype)  # (k_0, v_0, k_1, ...) rows, 8 guard columns
        call("fpnmt_rowsum_groups", code(dtype), n, B, T, d, tab, ptr(dc), ptr(lp), ptr(buf), buf.stride(0), 2 * d,
             sp())
        torch.cuda.synchronize()
        runs.append((dc, lp, buf))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    dc, lp, buf = runs[0]
    z64 = torch.stack([z.double().view(B, T, d) for z in dzs])
    err = (dc.double() - z64.sum(2)).abs()
    bound = T * 2.0 ** -24 * z64.abs().sum(2)
    print(f"rowsum max err {float(err.max()):.3e}, min slack {float((bound - err).min()):.3e}")
    assert bool((err <= bound).all())
    assert torch.equal(lp, dc.to(dtype))
    view = buf[:, :2 * n * d].view(B, n, 2, d)
    assert float(view[:, :, 0].abs().max()) == 0.0  # key blocks zeroed
    assert bool((view[:, :, 1] == 3.0).all()) and bool((buf[:, 2 * n * d:] == 3.0).all())  # nothing else touched


# ------------------------------------------------------------ decoder module
D_MODEL, HEADS, DFF, VOCAB, B, T, LAYERS = 128, 2, 256, 50, 3, 5, 2


def _decoder_run(dtype, rate, one_key, enc_len=1, masked=False, store_x=True):
    """One forward + backward of a fresh (same seed) Decoder; returns the
    output, d enc_output and every parameter gradient, as fp32 on the host."""
    import fpnmt
    from fpnmt import ops
    from fpnmt.layers import Init
    from models.transformer import Decoder, create_masks
    fpnmt.set_precision("fp32" if dtype == torch.float32 else "bf16")
    old = fpnmt.config.cross_one_key, fpnmt.config.cross_one_key_store_x
    fpnmt.config.cross_one_key, fpnmt.config.cross_one_key_store_x = one_key, store_x
    try:
        dec = Decoder(LAYERS, D_MODEL, HEADS, DFF, VOCAB, rate, max_seq_len=8,
                      init=Init(torch.Generator().manual_seed(11))).to(DEV)
        g = torch.Generator().manual_seed(3)
        tok = torch.randint(1, VOCAB, (B, T), generator=g).to(DEV)
        enc = torch.randn(B, enc_len, D_MODEL, generator=g).to(DEV).to(dtype).requires_grad_(True)
        w = torch.randn(B, T, D_MODEL, generator=g).to(DEV).to(dtype)
        pad = None
        if masked:
            pad = torch.zeros(B, 1, 1, enc_len, device=DEV)
        ops.runtime.reset_sites()
        out, attn = dec(tok, enc, True, create_masks(tok), pad)
        out.backward(w)
        torch.cuda.synchronize()
        res = {"out": out.detach().float().cpu(), "d_enc": enc.grad.detach().float().cpu(),
               "w2": attn["decoder_layer1_block2"].detach().float().cpu()}
        for name, prm in dec.named_parameters():
            res["grad:" + name] = (prm.grad if prm.grad is not None else torch.zeros_like(prm)).detach().float().cpu()
        return res
    finally:
        fpnmt.config.cross_one_key, fpnmt.config.cross_one_key_store_x = old
        fpnmt.set_precision("bf16")


def _is_qk(name):
    return ".mha2.wq." in name or ".mha2.wk." in name


@pytest.mark.parametrize("store_x", [True, False])
@pytest.mark.parametrize("rate", [0.1, 0.0])
def test_decoder_fast_equals_general_fp32(rate, store_x):
    """fp32 mode: only the summation order differs (dv = (sum_t dz) W^T
    against sum_t (dz W^T), the output-kernel gradient over B rows of sums
    against B*T rows): 1e-5 of each tensor's max. store_x: the LayerNorm
    backward reads the stored x (the default) or recomputes it."""
    gen = _decoder_run(torch.float32, rate, False)
    fast = _decoder_run(torch.float32, rate, True, store_x=store_x)
    assert torch.equal(fast["w2"], torch.ones(B, HEADS, T, 1))
    assert torch.equal(gen["w2"], fast["w2"])
    for k in gen:
        ref = float(gen[k].abs().max())
        if k.endswith(".mha1.wk.bias"):
            # exactly zero in exact arithmetic (a softmax does not move under a
            # shift common to all keys): what both paths store is the rounding
            # residue of the cancelling column sum of dk, so the scale is that
            # of the summed rows, taken from the same dk in the kernel gradient
            ref = float(gen[k.replace(".bias", ".kernel")].abs().max())
        err = float((gen[k] - fast[k]).abs().max())
        print(f"{k}: max {ref:.3e} err {err:.3e}")
        assert err <= 1e-5 * max(ref, 1e-30), k
        if k.startswith("grad:") and _is_qk(k):
            assert float(fast[k].abs().max()) == 0.0, k
    assert float(fast["grad:dec_layers.0.mha2.dense.kernel"].abs().max()) > 0
    assert float(fast["grad:dec_layers.1.mha2.wv.kernel"].abs().max()) > 0


def _rel_rms(a, ref):
    return float((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("rate", [0.1, 0.0])
def test_decoder_fast_vs_general_bf16(rate, parity_record):
    """bf16: both paths against the fp32-mode general path. The two bf16
    paths round at different points, so neither is the other's reference; the
    fast path's relative RMS error may exceed the general path's by at most
    25 %. The error of a path is the RMS, over the output, d enc_output and
    every parameter gradient with a non-zero reference, of that tensor's
    relative RMS error (single 128-element bias gradients scatter by more than
    the margin between two correct roundings; all tensors are printed)."""
    ref = _decoder_run(torch.float32, rate, False)
    gen = _decoder_run(torch.bfloat16, rate, False)
    fast = _decoder_run(torch.bfloat16, rate, True)
    eg, ef, qk_general = [], [], 0.0
    for k in ref:
        if k == "w2":
            continue
        if k.startswith("grad:") and _is_qk(k):
            assert float(fast[k].abs().max()) == 0.0, k
            qk_general = max(qk_general, float(gen[k].abs().max()))
            continue
        if float(ref[k].abs().max()) == 0.0 or k.endswith(".mha1.wk.bias"):
            continue  # no reference to be relative to (the self-attention key bias gradient is rounding residue)
        a, b = _rel_rms(gen[k], ref[k]), _rel_rms(fast[k], ref[k])
        print(f"{k}: general {a:.4e} fast {b:.4e}")
        eg.append(a)
        ef.append(b)
    e_gen = math.sqrt(sum(x * x for x in eg) / len(eg))
    e_fast = math.sqrt(sum(x * x for x in ef) / len(ef))
    print(f"rate {rate}: rel RMS error vs fp32 general: general bf16 {e_gen:.4e}, fast bf16 {e_fast:.4e}; "
          f"general path max |mha2 wq / wk gradient| {qk_general:.3e}")
    parity_record[f"cross_one_key_bf16_rate{rate}"] = {
        "general_rel_rms": e_gen, "fast_rel_rms": e_fast, "general_max_abs_mha2_qk_grad": qk_general}
    assert e_fast <= 1.25 * e_gen


# ------------------------------------------------------------------ routing
SCENARIOS = [("one_key", 1, False, True), ("recompute", 1, False, False), ("two_keys", 2, False, True),
             ("masked", 1, True, True)]


def _child(out_dir):
    """Every scenario with the switch off then on, in one process with the
    launch log set; the log lines each run appended are kept with its result."""
    log = os.environ["FPNMT_GEMM_LOG"]
    res = {}
    seen = 0
    for name, enc_len, masked, store_x in SCENARIOS:
        for on in (False, True):
            r = _decoder_run(torch.bfloat16, 0.1, on, enc_len, masked, store_x)
            lines = open(log).read().splitlines()
            r["log"], seen = lines[seen:], len(lines)
            res[(name, on)] = r
    torch.save(res, os.path.join(out_dir, "results.pt"))


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("cross_one_key")
    env = dict(os.environ, FPNMT_GEMM_LOG=str(out / "gemm.log"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True,
                       timeout=240)
    if r.returncode != 0:
        return {"error": f"child exited {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"}
    return torch.load(out / "results.pt")


def _fast_lines(lines):
    return [ln for ln in lines if ln.startswith(("ln_bcast", "rowsum_groups"))]


def test_routing_one_key_takes_fast_path(child):
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    assert not _fast_lines(child[("one_key", False)]["log"])
    fl = _fast_lines(child[("one_key", True)]["log"])
    assert sum(ln.startswith("ln_bcast op=fwd") for ln in fl) == LAYERS
    assert sum(ln.startswith("ln_bcast op=bwd") for ln in fl) == 0  # the backward reads the stored x
    assert sum(ln.startswith("rowsum_groups") for ln in fl) == 1
    rc = _fast_lines(child[("recompute", True)]["log"])
    assert sum(ln.startswith("ln_bcast op=bwd") for ln in rc) == LAYERS
    for k in child[("one_key", True)]:  # stored or recomputed x: the same bits
        if k != "log":
            assert torch.equal(child[("one_key", True)][k], child[("recompute", True)][k]), k
    # no attention launch is left for the cross-attention: one (self) per layer and pass
    on = [ln for ln in child[("one_key", True)]["log"] if ln.startswith("attn ")]
    off = [ln for ln in child[("one_key", False)]["log"] if ln.startswith("attn ")]
    assert len(off) - len(on) == 2 * LAYERS


@pytest.mark.parametrize("name", ["two_keys", "masked"])
def test_routing_general_path_unchanged(child, name):
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    off, on = child[(name, False)], child[(name, True)]
    assert not _fast_lines(on["log"]) and not _fast_lines(off["log"])
    for k in off:
        if k != "log":
            assert torch.equal(off[k], on[k]), k


# --------------------------------------------------------------------- step
def _steps(use_graph):
    import fpnmt
    from fpnmt.train import TrainEngine
    import test_gpu_model as TM
    m, _, _ = TM._build(num_layers=1, vocab=300, image=128, seed=17, rate=0.1)
    img, tok = TM._inputs(b=4, vocab=300, image=128, seed=23)
    fpnmt.set_precision("bf16")
    eng = TrainEngine(m, 1e-5, use_graph=use_graph)
    losses, flats = [], []
    for _ in range(3):
        losses.append(float(eng.step(img.to(DEV), tok.to(DEV))))
        torch.cuda.synchronize()
        flats.append(eng.arena.flat.detach().cpu().clone())
    return losses, flats


def test_step_graph_equals_eager_and_repeats():
    import fpnmt
    assert fpnmt.config.cross_one_key
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    eager, graph, again = _steps(False), _steps(True), _steps(True)
    assert all(math.isfinite(x) for x in eager[0])
    assert eager[0] == graph[0] == again[0]
    for a, b, c in zip(eager[1], graph[1], again[1]):
        assert torch.equal(a, b) and torch.equal(b, c)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "fpn-mt-image-captioning_amd"), root):
        if p not in sys.path:
            sys.path.insert(0, p)
    _child(sys.argv[1])
