"""Consensus decoding at BASELINE C5 (256 images, V = 10 000, 32 positions,
bf16) with 16 candidates per image, by the method of tools/beam_bench.py.

  launch: fpnmt_ciderd_consensus alone on 256 x 16 synthetic captions of 8 ..
          32 tokens over 200 words (so n-grams do repeat between an image's
          candidates), uniform and weighted, with and without the pair
          matrix: one captured graph of `--launches` launches, HIP events
          around `--replays` replays, the variants alternating for `--rounds`
          windows. Under a kernel trace (`rocprofv3 --kernel-trace --stats --
          python tools/consensus_bench.py launch --rounds 1`) the same
          launches give the kernel's own duration.
  decode: SampleDecoder (n_samples 16) and BeamDecoder (mode="beam", beam_n
          16) end to end (encoder + all positions + read-back), without
          consensus, with it (consensus_all, so both read every candidate
          back), and the host alternative: the plain decode's read-back plus
          utils.cider_reward.CiderDReward.consensus per image.
  census: one plain sample decode and one plain beam decode and nothing else
          (after a warm-up that captures the graphs), for a kernel trace:
          what a decode WITHOUT consensus launches.

Prints one JSON line per measurement. Run from the repository root:
  python tools/consensus_bench.py [launch] [decode] [census]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def corpus(rng, images, vocab, lo=6, hi=14):
    return [[rng.integers(4, vocab, size=int(rng.integers(lo, hi))).tolist() for _ in range(5)] for _ in range(images)]


def launch_bench(n_img, n, T, launches, replays, rounds):
    from fpnmt.cider_device import DeviceCiderD
    from fpnmt.train import capture_sequence
    rng = np.random.default_rng(0)
    tables = DeviceCiderD.from_corpus(corpus(rng, 500, 200), "cuda", max_len=T)
    R = n_img * n
    hist = np.zeros((R, T + 1), dtype=np.int32)
    lens = rng.integers(8, T + 1, size=R).astype(np.int32)
    for r in range(R):
        hist[r, 1:1 + lens[r]] = rng.integers(4, 200, size=lens[r])
    hist, lens = torch.from_numpy(hist).cuda(), torch.from_numpy(lens).cuda()
    fin = torch.zeros_like(lens)
    weight = torch.rand(R, dtype=torch.float64, device="cuda")
    util = torch.zeros(R, dtype=torch.float64, device="cuda")
    pick = torch.zeros(n_img, dtype=torch.int32, device="cuda")
    pair = torch.zeros(n_img * n * n, dtype=torch.float64, device="cuda")
    fns = {"uniform": lambda: tables.consensus(hist, lens, fin, n, util, pick),
           "weighted": lambda: tables.consensus(hist, lens, fin, n, util, pick, weight=weight),
           "weighted_with_pair": lambda: tables.consensus(hist, lens, fin, n, util, pick, weight=weight, pair=pair)}
    for fn in fns.values():
        fn()  # loads the code object outside the capture
    torch.cuda.synchronize()
    graphs = dict(zip(fns, capture_sequence([(lambda fn=fn: [fn() for _ in range(launches)]) for fn in fns.values()])))
    times = {k: [] for k in graphs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):  # round 0 warms up
        for name, gr in graphs.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(replays):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) * 1e3 / (replays * launches))
    out = {"measurement": f"fpnmt_ciderd_consensus, {n_img} images x {n} candidates of 8..{T} tokens, us per launch "
                          f"({launches} launches per graph, {replays} replays per window, {rounds} windows each, "
                          f"alternating)", "lds_bytes": tables.consensus_lds_bytes(n, T),
           "mean_utility": round(float(util.mean()), 4)}
    for name, ts in times.items():
        out[name] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2),
                     "max_us": round(max(ts), 2)}
    print(json.dumps(out), flush=True)


def _decoders(n_images, n, T, image, layers, V):
    import fpnmt
    from fpnmt.decode import BeamDecoder, SampleDecoder
    from fpnmt.layers import Init
    from models.transformer import Transformer
    fpnmt.set_precision("bf16")
    tr = Transformer(layers, 512, 8, 2048, math.ceil(image / 16) ** 2, V, 0.0, max_seq_len=T,
                     init=Init(torch.Generator().manual_seed(6))).cuda()
    imgs = torch.rand(n_images, image, image, 3, device="cuda") * 2 - 1
    return imgs, {"sample": SampleDecoder(tr, n_images, n, T, 2, 3, use_graph=True),
                  "beam": BeamDecoder(tr, n_images, n, T, 2, 3, use_graph=True, mode="beam")}


def decode_bench(n_images, n, T, image, layers, V, repeats):
    from fpnmt.cider_device import DeviceCiderD
    imgs, decs = _decoders(n_images, n, T, image, layers, V)
    tables = DeviceCiderD.from_corpus(corpus(np.random.default_rng(1), 1000, V), "cuda", max_len=T)
    host = tables.host

    def plain(m):
        return decs[m].decode(imgs, seed=7, check_every=0) if m == "sample" else \
            decs[m].decode(imgs, check_every=0, n_best=n)

    def device(m):
        kw = dict(consensus=tables, consensus_all=True, check_every=0)
        return decs[m].decode(imgs, seed=7, **kw) if m == "sample" else decs[m].decode(imgs, **kw)

    def on_host(m):
        return [host.consensus([ids for ids, _ in img]) for img in plain(m)]

    runs = {f"{m}_{k}": (lambda m=m, fn=fn: fn(m)) for m in decs
            for k, fn in (("plain", plain), ("consensus", device), ("host_consensus", on_host))}
    times = {k: [] for k in runs}
    with torch.no_grad():
        for rnd in range(repeats + 1):  # round 0 captures the graphs
            for name, fn in runs.items():
                if "host" in name and rnd > 2:
                    continue  # seconds per call: two timed calls
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"measurement": f"C5 decode end to end, {n_images} images x {n} candidates, {layers}L, V {V}, {T} positions, "
                          f"bf16, every candidate read back, ms per call ({repeats} calls each, alternating; the "
                          f"host alternative 2)"}
    for name, ts in times.items():
        out[name] = {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2),
                     "max_ms": round(max(ts), 2)}
    print(json.dumps(out), flush=True)


def census(n_images, n, T, image, layers, V):
    imgs, decs = _decoders(n_images, n, T, image, layers, V)
    with torch.no_grad():
        for _ in range(2):  # the first pass captures the graphs
            decs["sample"].decode(imgs, seed=7, check_every=0)
            decs["beam"].decode(imgs, check_every=0, n_best=n)
            torch.cuda.synchronize()
    print(json.dumps({"measurement": "two plain decodes per mode, for a kernel trace"}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", default=["launch", "decode"], choices=["launch", "decode", "census"])
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from fpnmt import _lib as L
    L.assert_in_tree()
    if "launch" in a.what:
        launch_bench(a.images, a.candidates, a.steps, a.launches, a.replays, a.rounds)
    if "decode" in a.what:
        decode_bench(a.images, a.candidates, a.steps, 224, 6, a.vocab, a.repeats)
    if "census" in a.what:
        census(a.images, a.candidates, a.steps, 224, 6, a.vocab)


if __name__ == "__main__":
    main()
