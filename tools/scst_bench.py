"""Self-critical training at the C2 shape (ResNet-50 FPN + 6 layers, V = 10 000,
224^2, 32 images, captions of 32 tokens, bf16) with n = 5 samples per image.

  step:   (a) the plain step at batch 32, (b) step_weighted at 32 x 5, (c) the
          naive alternative, the plain step on the 160 repeated images: each a
          captured graph, HIP events around `--replays` replays, the three
          alternating for `--rounds` windows; prints the medians and ranges.
  decode: (d) the sampled decode at 32 x 5, 31 positions, end to end with its
          read-back, and (e) the host's CIDEr-D reward of the 160 samples
          against 5 references per image (wall clock).
  xent:   (f) fpnmt_xent_fwd_bwd and fpnmt_xent_weighted_fwd_bwd alone at
          4 960 rows x V 10 000, each as one captured graph of `--launches`
          launches, alternating windows, in the same process.
  reward: (g) fpnmt_ciderd_reward and fpnmt_scst_pack alone at 160 rows x 31
          positions, 5 references per image, measured like (f).
  scst:   (h) the whole self-critical step end to end, the host-reward path
          against the device-reward path in the same run, alternating calls.

Expectations the numbers confirm or refute: (b) - (a) is the decoder side at
5 x the rows, so (b) is far below (c); in (f) the new kernel takes no longer
per row than the existing one (it reads the row once instead of three times).

Prints one JSON line per measurement. Run from the repository root:
  python tools/scst_bench.py [step] [decode] [xent]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fpn-mt-image-captioning_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _stats(ts, unit, nd=3):
    return {f"median_{unit}": round(statistics.median(ts), nd), f"min_{unit}": round(min(ts), nd),
            f"max_{unit}": round(max(ts), nd), f"windows_{unit}": [round(x, nd) for x in ts]}


def _model(layers, V, T, image, seed):
    from fpnmt.layers import Init
    from models.transformer import Transformer
    return Transformer(layers, 512, 8, 2048, math.ceil(image / 16) ** 2, V, 0.1, max_seq_len=T,
                       init=Init(torch.Generator().manual_seed(seed))).cuda()


def _captions(rows, T, V, g):
    tok = torch.randint(4, V, (rows, T), generator=g)
    tok[:, 0] = 2
    for r in range(rows):
        n = int(torch.randint(8, T + 1, (1,), generator=g))
        tok[r, n - 1] = 3
        tok[r, n:] = 0
    return tok.cuda()


def step_bench(B, n, T, V, image, layers, replays, rounds):
    import fpnmt
    from fpnmt.train import TrainEngine
    fpnmt.set_precision("bf16")
    g = torch.Generator().manual_seed(0)
    img = (torch.rand(B, image, image, 3, generator=g) * 2 - 1).cuda()
    tok1, tokn = _captions(B, T, V, g), _captions(B * n, T, V, g)
    w = torch.randn(B * n, generator=g).cuda()
    rep = img.repeat_interleave(n, 0).contiguous()
    e1 = TrainEngine(_model(layers, V, T, image, 1), 1e-6, use_graph=True)  # (a) and (b): one engine, one arena
    e2 = TrainEngine(_model(layers, V, T, image, 1), 1e-6, use_graph=True)  # (c)
    fns = {"a_plain_b32": lambda: e1.step(img, tok1),
           "b_weighted_32x5": lambda: e1.step_weighted(img, tokn, w),
           "c_plain_b160_repeated": lambda: e2.step(rep, tokn)}
    for fn in fns.values():  # eager, capture, one replay
        for _ in range(3):
            loss = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):  # round 0 warms up
        for name, fn in fns.items():
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(replays):
                loss = fn()
            ev1.record()
            torch.cuda.synchronize()
            assert math.isfinite(float(loss)), name
            if rnd:
                times[name].append(ev0.elapsed_time(ev1) / replays)
    out = {"measurement": f"training step, {layers}L V {V} {image}^2 T {T} bf16, {B} images, n = {n}; ms per step "
                          f"({replays} graph replays per window, {rounds} windows each, alternating)"}
    out.update({k: _stats(ts, "ms") for k, ts in times.items()})
    print(json.dumps(out), flush=True)
    fpnmt.set_precision("fp32")


def decode_bench(B, n, T, V, image, layers, repeats):
    import fpnmt
    from fpnmt.decode import SampleDecoder
    from utils.cider_reward import CiderDReward
    fpnmt.set_precision("bf16")
    tr = _model(layers, V, T, image, 2)
    with torch.no_grad():
        tr.final_layer.bias[3] += 4.0  # random weights would never end a caption
    from fpnmt.layers import invalidate_weights
    invalidate_weights()
    img = torch.rand(B, image, image, 3, device="cuda") * 2 - 1
    dec = SampleDecoder(tr, B, n, T - 1, 2, 3, use_graph=True)
    g = torch.Generator().manual_seed(3)
    refs = [[torch.randint(4, V // 50, (int(torch.randint(8, 14, (1,), generator=g)),), generator=g).tolist()
             for _ in range(5)] for _ in range(B)]
    t_dec, t_build, t_score, lens = [], [], [], []
    with torch.no_grad():
        for rnd in range(repeats + 1):  # round 0 captures the graphs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            drawn = dec.decode(img)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rw = CiderDReward.from_corpus(refs)
            t2 = time.perf_counter()
            r = rw.score(list(range(B)), [[s[0] for s in per] for per in drawn])
            t3 = time.perf_counter()
            if rnd:
                t_dec.append((t1 - t0) * 1e3)
                t_build.append((t2 - t1) * 1e3)
                t_score.append((t3 - t2) * 1e3)
                lens.append(sum(len(s[0]) for per in drawn for s in per) / (B * n))
    assert r.shape == (B * n,)
    out = {"measurement": f"sampled decode {B} x {n}, {T - 1} positions, {layers}L V {V} bf16, end to end, and the host "
                          f"CIDEr-D reward of its {B * n} samples against 5 references per image; ms per call "
                          f"({repeats} calls)",
           "d_sample_decode": _stats(t_dec, "ms"), "e_reward_from_corpus": _stats(t_build, "ms"),
           "e_reward_score": _stats(t_score, "ms"), "mean_sample_len": round(statistics.mean(lens), 2)}
    print(json.dumps(out), flush=True)
    fpnmt.set_precision("fp32")


def xent_bench(rows, V, w_div, launches, replays, rounds):
    from fpnmt import _lib as L
    from fpnmt.train import capture_sequence
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(rows, V, generator=g) * 3).cuda()
    lab = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    lab[torch.rand(rows, generator=g) < 0.35] = 0  # the pad share of padded captions
    lab = lab.cuda()
    w = torch.randn(rows // w_div, generator=g).cuda()
    loss = torch.zeros(1, device="cuda")
    logp = torch.zeros(rows, device="cuda")
    dlog = torch.empty(rows, V, device="cuda")

    def plain():
        L.call("fpnmt_xent_fwd_bwd", L.F32, rows, V, logits.data_ptr(), V, lab.data_ptr(), loss.data_ptr(),
               dlog.data_ptr(), V, 1.0, L.stream_ptr())

    def weighted(with_logp):
        def fn():
            L.call("fpnmt_xent_weighted_fwd_bwd", L.F32, rows, V, logits.data_ptr(), V, lab.data_ptr(), w.data_ptr(),
                   w_div, loss.data_ptr(), logp.data_ptr() if with_logp else None, dlog.data_ptr(), V, 1.0,
                   L.stream_ptr())
        return fn

    fns = {"xent_fwd_bwd": plain, "xent_weighted_fwd_bwd": weighted(False),
           "xent_weighted_fwd_bwd_row_logp": weighted(True)}
    for fn in fns.values():
        fn()  # loads the code object outside the capture
    torch.cuda.synchronize()
    graphs = dict(zip(fns, capture_sequence([(lambda fn=fn: [fn() for _ in range(launches)]) for fn in fns.values()])))
    times = {k: [] for k in graphs}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):
        for name, gr in graphs.items():
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(replays):
                gr.replay()
            ev1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(ev0.elapsed_time(ev1) * 1e3 / (replays * launches))
    live = float((lab != 0).float().mean())
    out = {"measurement": f"loss kernels alone, {rows} rows x V {V} fp32 logits and gradient ({live:.2f} of the rows "
                          f"live), us per launch with its ordered sum ({launches} launches per graph, {replays} replays "
                          f"per window, {rounds} windows each, alternating)"}
    for name, ts in times.items():
        out[name] = _stats(ts, "us", 2)
        out[name]["ns_per_row"] = round(statistics.median(ts) * 1e3 / rows, 2)
    print(json.dumps(out), flush=True)


def _refs(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randint(4, V // 50, (int(torch.randint(8, 14, (1,), generator=g)),), generator=g).tolist()
             for _ in range(5)] for _ in range(B)]


def reward_bench(B, n, T, V, launches, replays, rounds):
    """(g) fpnmt_ciderd_reward and fpnmt_scst_pack alone: B * n rows of T - 1
    positions as a sampler leaves them (lengths 8 .. T - 1, tokens from the
    references' vocabulary), 5 references per image."""
    from fpnmt import _lib as L
    from fpnmt.cider_device import DeviceCiderD
    from fpnmt.train import capture_sequence
    refs = _refs(B, V, 3)
    table = DeviceCiderD.from_corpus(refs, "cuda", max_len=T - 1)
    g = torch.Generator().manual_seed(5)
    R, steps = B * n, T - 1
    hist = torch.randint(4, V // 50, (R, T), generator=g, dtype=torch.int32)
    hist[:, 0] = 2
    lens = torch.randint(8, steps + 1, (R,), generator=g, dtype=torch.int32)
    fin = (lens < steps).int()
    for r in range(R):
        if fin[r]:
            hist[r, 1 + int(lens[r]):] = 3
    slen = lens + fin
    hist, slen, fin = hist.cuda(), slen.cuda(), fin.cuda()
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    reward = torch.zeros(R, dtype=torch.float64, device="cuda")
    score = -torch.rand(R, device="cuda") * 30
    tok = torch.zeros((R, T), dtype=torch.int64, device="cuda")
    adv = torch.zeros(R, device="cuda")
    sc = torch.zeros(3, dtype=torch.float64, device="cuda")

    def f_reward():
        table.reward(hist, slen, fin, idx, n, reward)

    def f_pack():
        L.call("fpnmt_scst_pack", B, n, L.SCST_MEAN, reward.data_ptr(), None, hist.data_ptr(), T, slen.data_ptr(),
               fin.data_ptr(), score.data_ptr(), 2, 3, steps, tok.data_ptr(), T, adv.data_ptr(), sc.data_ptr(),
               L.stream_ptr())

    fns = {"ciderd_reward": f_reward, "scst_pack": f_pack}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert float(reward.sum()) > 0 and int(tok[:, 0].sum()) == 2 * R
    graphs = dict(zip(fns, capture_sequence([(lambda fn=fn: [fn() for _ in range(launches)]) for fn in fns.values()])))
    times = {k: [] for k in graphs}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):
        for name, gr in graphs.items():
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(replays):
                gr.replay()
            ev1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(ev0.elapsed_time(ev1) * 1e3 / (replays * launches))
    out = {"measurement": f"reward kernels alone, {R} rows x {steps} positions, 5 references per image, "
                          f"{len(table.np['df_keys'])} document n-grams; us per launch ({launches} launches per graph, "
                          f"{replays} replays per window, {rounds} windows each, alternating)"}
    out.update({k: _stats(ts, "us", 2) for k, ts in times.items()})
    print(json.dumps(out), flush=True)


def scst_step_bench(B, n, T, V, image, layers, repeats):
    """(h) the whole self-critical step, end to end (host clock around the
    call and a device synchronise): the host-reward path (CiderDReward built
    once over the references, behind a callable) against the device-reward
    path (DeviceCiderD), two identically built models, alternating calls."""
    import fpnmt
    from fpnmt.cider_device import DeviceCiderD
    from fpnmt.layers import invalidate_weights
    from fpnmt.scst import SelfCriticalTrainer
    from fpnmt.train import TrainEngine
    from utils.cider_reward import CiderDReward
    fpnmt.set_precision("bf16")
    refs = _refs(B, V, 3)
    host = CiderDReward.from_corpus(refs)
    table = DeviceCiderD.from_corpus(refs, "cuda", max_len=T - 1)
    img = torch.rand(B, image, image, 3, device="cuda") * 2 - 1
    trainers = {}
    for name in ("host_reward", "device_reward"):
        tr = _model(layers, V, T, image, 2)
        with torch.no_grad():
            tr.final_layer.bias[3] += 4.0  # random weights would never end a caption
        invalidate_weights()
        trainers[name] = SelfCriticalTrainer(tr, TrainEngine(tr, 1e-6, use_graph=True), 2, 3, T)
    rewards = {"host_reward": lambda i, c: host(i, c), "device_reward": table}
    times = {k: [] for k in trainers}
    for rnd in range(repeats + 2):  # rounds 0 and 1: eager, then the captures
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tr.step(img, None, n_samples=n, reward=rewards[name], seed=rnd)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rnd >= 2:
                times[name].append((t1 - t0) * 1e3)
        assert math.isfinite(float(out["loss"]))
    out = {"measurement": f"self-critical step end to end, {layers}L V {V} {image}^2 T {T} bf16, {B} images, n = {n}, "
                          f"5 references per image; ms per step (host clock, {repeats} calls each, alternating)"}
    out.update({k: _stats(ts, "ms") for k, ts in times.items()})
    print(json.dumps(out), flush=True)
    fpnmt.set_precision("fp32")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", default=["step", "decode", "xent"],
                    choices=["step", "decode", "xent", "reward", "scst"])
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from fpnmt import _lib as L
    L.assert_in_tree()
    if "xent" in a.what:
        xent_bench(a.images * a.samples * (a.seq - 1), a.vocab, a.seq - 1, a.launches, a.replays, a.rounds)
    if "reward" in a.what:
        reward_bench(a.images, a.samples, a.seq, a.vocab, a.launches, a.replays, a.rounds)
    if "scst" in a.what:
        scst_step_bench(a.images, a.samples, a.seq, a.vocab, 224, a.layers, a.repeats)
    if "decode" in a.what:
        decode_bench(a.images, a.samples, a.seq, a.vocab, 224, a.layers, a.repeats)
    if "step" in a.what:
        step_bench(a.images, a.samples, a.seq, a.vocab, 224, a.layers, a.replays, a.rounds)


if __name__ == "__main__":
    main()
