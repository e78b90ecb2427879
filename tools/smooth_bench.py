"""Label-smoothed step, eval_step and the two loss kernels at BASELINE C2
(ResNet-50 FPN, 6 layers, V = 10 000, batch 32, 224 x 224, bf16, graphs).

  step:    TrainEngine.step at label_smoothing 0 and 0.1 (two engines on two
           copies of one model), windows of `--steps` replays alternating
           between the two for `--rounds` rounds, HIP events around each
           window; prints every window, the medians, and per setting the
           spread (max - min) of its own windows: what two runs of the same
           setting differ by.
  eval:    TrainEngine.eval_step (graph replay) at the same shape, timed the
           same way.
  xent:    fpnmt_xent_fwd_bwd (the three-pass kernel of the eps = 0 step)
           and fpnmt_xent_smooth_fwd_bwd with and without a gradient, alone
           on 992 x 10 000 fp32 logits, each as a captured graph of
           `--launches` launches; us per launch and the fraction of the HBM
           peak for the bytes the kernel must move (logits in, gradient out).
  profile: a few replayed steps of both settings and a few eval_step replays
           and nothing else, to run under the profiler in a run of its own:
             rocprofv3 --kernel-trace --stats -d <dir> -- python tools/smooth_bench.py profile
           (xent_kernel is the old loss kernel, xent_smooth_kernel the new).

Prints one JSON line per measurement. Run from the repository root:
  python tools/smooth_bench.py [step] [eval] [xent]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fpn-mt-image-captioning_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def _batch(b, image, vocab, T, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(b, image, image, 3, generator=g) * 2 - 1
    tok = torch.randint(4, vocab, (b, T), generator=g, dtype=torch.int64)
    tok[:, 0] = 2
    lens = torch.randint(8, T + 1, (b,), generator=g)
    for i in range(b):
        n = int(lens[i])
        tok[i, n - 1] = 3
        tok[i, n:] = 0
    return img.cuda(), tok.to(torch.int32).cuda()


def _engine(a, eps):
    import fpnmt
    from fpnmt.layers import Init
    from fpnmt.train import TrainEngine
    from models.transformer import Transformer
    from utils.utils import CustomSchedule
    fpnmt.set_precision("bf16")
    m = Transformer(a.layers, 512, 8, 2048, math.ceil(a.image / 16) ** 2, a.vocab, 0.0, max_seq_len=a.T,
                    init=Init(torch.Generator().manual_seed(1234))).cuda()
    return TrainEngine(m, CustomSchedule(2048, 4000), use_graph=True, label_smoothing=eps)


def _windows(fns, calls, rounds):
    """ms per call of every fn, windows of `calls` calls alternating between them."""
    times = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):  # round 0 warms up
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / calls)
    return times


def _summary(ts, unit="ms", scale=1.0, digits=3):
    ts = [t * scale for t in ts]
    return {f"median_{unit}": round(statistics.median(ts), digits), f"min_{unit}": round(min(ts), digits),
            f"max_{unit}": round(max(ts), digits), f"spread_{unit}": round(max(ts) - min(ts), digits),
            f"windows_{unit}": [round(t, digits) for t in ts]}


def step_bench(a):
    img, tok = _batch(a.batch, a.image, a.vocab, a.T, 1000)
    engines = {"eps_0": _engine(a, 0.0), "eps_0.1": _engine(a, 0.1)}
    for e in engines.values():
        for _ in range(3):  # eager, capture, replay
            e.step(img, tok)
    times = _windows({k: (lambda e=e: e.step(img, tok)) for k, e in engines.items()}, a.steps, a.rounds)
    out = {"measurement": f"C2 step, {a.layers}L V {a.vocab} batch {a.batch} {a.image}^2 bf16 graphs, ms per step "
                          f"({a.steps} steps per window, {a.rounds} windows each, alternating)"}
    for k, ts in times.items():
        out[k] = _summary(ts)
    d = out["eps_0.1"]["median_ms"] - out["eps_0"]["median_ms"]
    out["eps_0.1_minus_eps_0_ms"] = round(d, 3)
    out["same_setting_spread_ms"] = max(out["eps_0"]["spread_ms"], out["eps_0.1"]["spread_ms"])
    print(json.dumps(out), flush=True)


def eval_bench(a):
    img, tok = _batch(a.batch, a.image, a.vocab, a.T, 1000)
    eng = _engine(a, 0.1)
    for _ in range(3):
        eng.eval_step(img, tok)
    times = _windows({"eval_step": lambda: eng.eval_step(img, tok)}, a.steps, a.rounds)
    out = {"measurement": f"C2 eval_step, {a.layers}L V {a.vocab} batch {a.batch} {a.image}^2 bf16 graph, ms per call "
                          f"({a.steps} calls per window, {a.rounds} windows)",
           "eval_step": _summary(times["eval_step"])}
    print(json.dumps(out), flush=True)


def xent_bench(a):
    from fpnmt import _lib as L
    from fpnmt.train import capture_sequence
    rows, V = a.batch * (a.T - 1), a.vocab
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(rows, V, generator=g) * 3).cuda()
    _, tok = _batch(a.batch, 8, V, a.T, 1000)
    lab = tok[:, 1:].contiguous().view(-1)
    loss = torch.zeros(1, device="cuda")
    dlog = torch.empty(rows, V, device="cuda")
    logp = torch.empty(rows, device="cuda")
    hit = torch.empty(rows, dtype=torch.int32, device="cuda")

    def plain():
        L.call("fpnmt_xent_fwd_bwd", L.F32, rows, V, logits.data_ptr(), V, lab.data_ptr(), loss.data_ptr(),
               dlog.data_ptr(), V, 1.0, L.stream_ptr())

    def smooth(grad, stats):
        def f():
            L.call("fpnmt_xent_smooth_fwd_bwd", L.F32, rows, V, logits.data_ptr(), V, lab.data_ptr(), 0.1,
                   loss.data_ptr(), logp.data_ptr() if stats else None, hit.data_ptr() if stats else None,
                   dlog.data_ptr() if grad else None, V, 1.0, L.stream_ptr())
        return f

    fns = {"xent_fwd_bwd": plain, "xent_smooth_fwd_bwd": smooth(True, False),
           "xent_smooth_eval_no_gradient": smooth(False, True)}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    graphs = dict(zip(fns, capture_sequence([(lambda fn=fn: [fn() for _ in range(a.launches)]) for fn in fns.values()])))
    times = _windows({k: gr.replay for k, gr in graphs.items()}, a.replays, a.rounds)
    live = int((lab != 0).sum())
    out = {"measurement": f"loss kernels alone, {rows} x {V} fp32 ({live} live rows), us per launch with its ordered "
                          f"sum ({a.launches} launches per graph, {a.replays} replays per window, {a.rounds} windows "
                          "each, alternating)"}
    for k, ts in times.items():
        out[k] = _summary(ts, "us", 1e3 / a.launches, 2)
        # a live row's logits in (+ its gradient out); a pad row is a zero fill of its gradient
        nbytes = 4 * V * (live + (rows if "no_gradient" not in k else 0))
        out[k]["min_bytes_MB"] = round(nbytes / 1e6, 2)
        out[k]["fraction_of_hbm_peak"] = round(nbytes / (out[k]["median_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 3)
    print(json.dumps(out), flush=True)


def profile_run(a):
    img, tok = _batch(a.batch, a.image, a.vocab, a.T, 1000)
    for eps in (0.0, 0.1):
        eng = _engine(a, eps)
        for _ in range(2 + a.steps):
            eng.step(img, tok)
        if eps:
            for _ in range(2 + a.steps):
                eng.eval_step(img, tok)
        torch.cuda.synchronize()
        del eng
    print(json.dumps({"profile": f"{a.steps} replayed steps at eps 0 and 0.1, {a.steps} eval_step replays"}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", default=["step", "eval", "xent"], choices=["step", "eval", "xent", "profile"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    a = ap.parse_args()
    from fpnmt import _lib as L
    L.assert_in_tree()
    for what, fn in (("step", step_bench), ("eval", eval_bench), ("xent", xent_bench), ("profile", profile_run)):
        if what in a.what:
            fn(a)


if __name__ == "__main__":
    main()
