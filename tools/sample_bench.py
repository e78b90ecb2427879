"""Sampled decoding at BASELINE C5 (2048 rows = 256 images x 8, V = 10 000, bf16).

  step:   fpnmt_sample_step unfiltered, with top_k = 50, with top_p = 0.9 and
          with both, against fpnmt_beam_step_log at 256 x 8 on the same
          logits, each as one captured graph of `--launches` launches (an
          8 KB copy before each launch puts the scores back, as in
          tools/beam_bench.py; <end> is made improbable so no row finishes
          and every launch does the full work), HIP events around
          `--replays` replays, the kernels alternating for `--rounds`
          windows; prints every window, the medians and the spread.
  decode: SampleDecoder (n_samples = 8) against BeamDecoder mode="beam" end
          to end (encoder + all steps + result read-back), timed as bench.py
          times C5.

Prints one JSON line per measurement. Run from the repository root:
  python tools/sample_bench.py [step] [decode]
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

VARIANTS = {"sample_plain": (0, 1.0), "sample_top_k50": (50, 1.0), "sample_top_p0.9": (0, 0.9),
            "sample_top_k50_top_p0.9": (50, 0.9)}


def step_bench(n_img, K, V, T, t, launches, replays, rounds):
    from fpnmt import _lib as L
    from fpnmt.train import capture_sequence
    R = n_img * K
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(R, V, generator=g)
    end = V - 1
    logits[:, end] = -60.0  # <end> is never drawn or ranked: rows stay live, every launch does the full work
    logits = logits.cuda()
    hist = [torch.randint(4, V, (R, T + 1), generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    src = [torch.randint(0, R, (R, T), generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    tok = torch.zeros(R, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_img, dtype=torch.int32, device="cuda")
    score = torch.empty(R, device="cuda")
    blen = torch.zeros(R, dtype=torch.int32, device="cuda")
    fin = torch.zeros(R, dtype=torch.int32, device="cuda")
    kept = torch.zeros(R, dtype=torch.int32, device="cuda")
    word = torch.ones(1, dtype=torch.int64, device="cuda")
    score0 = (-torch.rand(R, generator=g) * 4 - 10).cuda()

    def log(i):
        score.copy_(score0)
        L.call("fpnmt_beam_step_log", n_img, K, V, logits.data_ptr(), V, score.data_ptr(), blen.data_ptr(),
               fin.data_ptr(), hist[i % 2].data_ptr(), hist[(i + 1) % 2].data_ptr(), T + 1, t,
               src[i % 2].data_ptr(), src[(i + 1) % 2].data_ptr(), T, end, tok.data_ptr(), status.data_ptr(),
               L.stream_ptr())

    def sample(top_k, top_p):
        def fn(i):
            score.copy_(score0)
            L.call("fpnmt_sample_step", R, V, logits.data_ptr(), V, 1.0, top_k, top_p, i, word.data_ptr(),
                   score.data_ptr(), blen.data_ptr(), fin.data_ptr(), hist[0].data_ptr(), T + 1, t, end,
                   tok.data_ptr(), kept.data_ptr(), L.stream_ptr())
        return fn

    fns = {"beam_step_log": log}
    fns.update({name: sample(*kp) for name, kp in VARIANTS.items()})
    mean_kept = {}
    for name, fn in fns.items():
        fn(0)  # loads the code object outside the capture
        torch.cuda.synchronize()
        if name in VARIANTS:
            mean_kept[name] = round(float(kept.float().mean()), 1)
    graphs = dict(zip(fns, capture_sequence([(lambda fn=fn: [fn(i) for i in range(launches)]) for fn in fns.values()])))
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
    assert int(status.sum()) == 0 and int(fin.sum()) == 0, "rows finished: the launches did not all do the full work"
    out = {"measurement": f"sample step against beam_step_log, {R} rows ({n_img} x {K}) x V {V}, t {t}, us per launch "
                          f"with its 8 KB state copy ({launches} launches per graph, {replays} replays per window, "
                          f"{rounds} windows each, alternating)"}
    for name, ts in times.items():
        out[name] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2),
                     "max_us": round(max(ts), 2), "windows_us": [round(x, 2) for x in ts]}
        if name in mean_kept:
            out[name]["mean_kept"] = mean_kept[name]
    print(json.dumps(out), flush=True)


def decode_bench(n_images, K, T, image, layers, V, repeats):
    import fpnmt
    from fpnmt.decode import BeamDecoder, SampleDecoder
    from fpnmt.layers import Init
    from models.transformer import Transformer
    fpnmt.set_precision("bf16")
    tr = Transformer(layers, 512, 8, 2048, math.ceil(image / 16) ** 2, V, 0.0, max_seq_len=T,
                     init=Init(torch.Generator().manual_seed(6))).cuda()
    imgs = torch.rand(n_images, image, image, 3, device="cuda") * 2 - 1
    decs = {"beam": BeamDecoder(tr, n_images, K, T, 2, 3, use_graph=True, mode="beam"),
            "sample": SampleDecoder(tr, n_images, K, T, 2, 3, use_graph=True),
            "sample_top_k50_top_p0.9": SampleDecoder(tr, n_images, K, T, 2, 3, use_graph=True, top_k=50, top_p=0.9)}
    times = {m: [] for m in decs}
    outs = {}
    with torch.no_grad():
        for rnd in range(repeats + 1):  # round 0 captures the graphs
            for m, dec in decs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[m] = dec.decode(imgs, check_every=0)
                torch.cuda.synchronize()
                if rnd:
                    times[m].append((time.perf_counter() - t0) * 1e3)
    out = {"measurement": f"C5 decode end to end, {n_images} images x {K} beams / samples, {layers}L, V {V}, {T} steps, "
                          f"bf16, ms per call ({repeats} calls each, alternating)"}
    for m, ts in times.items():
        out[m] = {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2),
                  "max_ms": round(max(ts), 2)}
    for m in decs:
        if m != "beam":
            caps = [tuple(ids) for img in outs[m] for ids, _ in img]
            out[m]["mean_len"] = round(sum(len(c) for c in caps) / len(caps), 2)
            out[m]["distinct_captions_per_image"] = round(
                sum(len({tuple(ids) for ids, _ in img}) for img in outs[m]) / n_images, 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", default=["step", "decode"], choices=["step", "decode"])
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from fpnmt import _lib as L
    L.assert_in_tree()
    if "step" in a.what:
        step_bench(a.images, a.samples, a.vocab, a.steps, 5, a.launches, a.replays, a.rounds)
    if "decode" in a.what:
        decode_bench(a.images, a.samples, a.steps, 224, 6, a.vocab, a.repeats)


if __name__ == "__main__":
    main()
