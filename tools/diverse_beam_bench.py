"""Diverse beam search at BASELINE C5 (256 images x 8 beams, V = 10 000,
bf16), by the method of tools/beam_bench.py.

  step:   fpnmt_beam_step_log and fpnmt_beam_step_groups at G = 2, 4, 8
          (diversity_penalty 0.5) on the same logits, each as one captured
          graph of `--launches` launches (ping-ponging the history tables; an
          8 KB copy before each launch puts the scores back, so every launch
          ranks the same candidates), HIP events around `--replays` replays,
          the kernels alternating for `--rounds` windows. The rows of an image
          are one base row plus a little noise per row, so the groups compete
          for the same tokens and the penalty list is in use (independent
          random rows would never hit the filter).
  decode: BeamDecoder end to end (encoder + all steps + result read-back) in
          mode="beam" and with beam_groups = 4, timed as bench.py times C5.

Prints one JSON line per measurement. Run from the repository root:
  python tools/diverse_beam_bench.py [step] [decode]
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


def step_bench(n_img, K, V, T, t, groups, lam, launches, replays, rounds):
    from fpnmt import _lib as L
    from fpnmt.train import capture_sequence
    R = n_img * K
    g = torch.Generator().manual_seed(0)
    logits = (2 * torch.randn(n_img, 1, V, generator=g) + 0.05 * torch.randn(n_img, K, V, generator=g)).reshape(R, V)
    end = V - 1
    logits[:, end] = -30.0  # <end> never ranks: beams stay live, every launch does the full work
    logits = logits.contiguous().cuda()
    hist = [torch.randint(4, V, (R, T + 1), generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    src = [torch.randint(0, R, (R, T), generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    tok = torch.zeros(R, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_img, dtype=torch.int32, device="cuda")
    score = torch.empty(R, device="cuda")
    blen = torch.zeros(R, dtype=torch.int32, device="cuda")
    fin = torch.zeros(R, dtype=torch.int32, device="cuda")
    score0 = (-torch.rand(R, generator=g) * 0.1 - 10).cuda()

    def tail(i):
        return (logits.data_ptr(), V, score.data_ptr(), blen.data_ptr(), fin.data_ptr(), hist[i % 2].data_ptr(),
                hist[(i + 1) % 2].data_ptr(), T + 1, t, src[i % 2].data_ptr(), src[(i + 1) % 2].data_ptr(), T, end,
                tok.data_ptr(), status.data_ptr(), L.stream_ptr())

    def log(i):
        score.copy_(score0)
        L.call("fpnmt_beam_step_log", n_img, K, V, *tail(i))

    def grouped(G):
        def fn(i):
            score.copy_(score0)
            L.call("fpnmt_beam_step_groups", n_img, K, G, lam, V, *tail(i))
        return fn

    fns = {"beam_step_log": log}
    fns.update({f"beam_step_groups_G{G}": grouped(G) for G in groups})
    toks = {}
    for name, fn in fns.items():
        fn(0)  # loads the code object outside the capture
        torch.cuda.synchronize()
        toks[name] = tok.cpu().clone()
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
    assert int(status.sum()) == 0 and int(fin.sum()) == 0, "beams finished: the launches did not all do the full work"
    out = {"measurement": f"beam step kernels, {n_img} images x {K} beams x V {V}, t {t}, diversity_penalty {lam}, "
                          f"us per launch with its 8 KB state copy ({launches} launches per graph, {replays} replays "
                          f"per window, {rounds} windows each, alternating)"}
    for name, ts in times.items():
        out[name] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2),
                     "max_us": round(max(ts), 2), "windows_us": [round(x, 2) for x in ts],
                     "slots_differing_from_beam_step_log": int((toks[name] != toks["beam_step_log"]).sum())}
    print(json.dumps(out), flush=True)


def decode_bench(n_images, K, T, image, layers, V, G, lam, repeats):
    import fpnmt
    from fpnmt.decode import BeamDecoder
    from fpnmt.layers import Init
    from models.transformer import Transformer
    fpnmt.set_precision("bf16")
    tr = Transformer(layers, 512, 8, 2048, math.ceil(image / 16) ** 2, V, 0.0, max_seq_len=T,
                     init=Init(torch.Generator().manual_seed(6))).cuda()
    imgs = torch.rand(n_images, image, image, 3, device="cuda") * 2 - 1
    decs = {"beam": BeamDecoder(tr, n_images, K, T, 2, 3, use_graph=True, mode="beam"),
            f"beam_groups_{G}": BeamDecoder(tr, n_images, K, T, 2, 3, use_graph=True, mode="beam", beam_groups=G,
                                            diversity_penalty=lam)}
    times = {m: [] for m in decs}
    outs = {}
    with torch.no_grad():
        for rnd in range(repeats + 1):  # round 0 captures the graphs
            for m, dec in decs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[m] = dec.decode(imgs, check_every=0, n_best=K)
                torch.cuda.synchronize()
                if rnd:
                    times[m].append((time.perf_counter() - t0) * 1e3)
    out = {"measurement": f"C5 decode end to end, {n_images} images x {K} beams, {layers}L, V {V}, {T} steps, bf16, "
                          f"diversity_penalty {lam}, ms per call ({repeats} calls each, alternating)"}
    for m, ts in times.items():
        firsts = [len({tuple(ids[:2]) for ids, _ in img}) for img in outs[m]]
        out[m] = {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2),
                  "max_ms": round(max(ts), 2), "mean_distinct_first_two_tokens": round(sum(firsts) / n_images, 2)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", default=["step", "decode"], choices=["step", "decode"])
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--beams", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--decode-groups", type=int, default=4)
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from fpnmt import _lib as L
    L.assert_in_tree()
    if "step" in a.what:
        step_bench(a.images, a.beams, a.vocab, a.steps, 5, a.groups, a.penalty, a.launches, a.replays, a.rounds)
    if "decode" in a.what:
        decode_bench(a.images, a.beams, a.steps, 224, 6, a.vocab, a.decode_groups, a.penalty, a.repeats)


if __name__ == "__main__":
    main()
