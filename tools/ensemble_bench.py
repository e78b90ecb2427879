"""Ensemble decoding at BASELINE C5 (256 images x 8 beams, V = 10 000, bf16).

  kernel: fpnmt_logits_ensemble for M = 2 and 4 in both modes on (2048, 10000)
          fp32 rows, beside the project's other launches that stream logits
          rows, fpnmt_logits_constrain and fpnmt_beam_step_log, on the same
          rows: each as one captured graph of `--launches` launches, HIP
          events around `--replays` replays, all alternating for `--rounds`
          windows. Prints us per launch and, for the combine, the achieved
          bytes per second over its algorithmic bytes rows * vocab * 4 * (M + 1).
  decode: BeamDecoder mode="beam" end to end (encoders + all steps + result
          read-back) with one model and with ensembles of M = 2 and 4 models
          of the C5 geometry, alternating; the ratio to M single decodes.

Prints one JSON line per measurement. Run from the repository root:
  python tools/ensemble_bench.py [kernel] [decode]
"""
import argparse
import ctypes as C
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


def kernel_bench(n_img, K, V, T, t, launches, replays, rounds):
    from fpnmt import _lib as L
    from fpnmt.train import capture_sequence
    R = n_img * K
    g = torch.Generator().manual_seed(0)
    rows = [(torch.randn(R, V, generator=g) * 4).cuda() for _ in range(4)]
    end = V - 1
    for x in rows:
        x[:, end] = -30.0  # <end> never ranks: the beams stay live, every launch does the full work
    out = torch.empty(R, V, device="cuda")
    work = rows[0].clone()
    hist = [torch.randint(4, V, (R, T + 1), generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    src = [torch.randint(0, R, (R, T), generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    tok = torch.zeros(R, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_img, dtype=torch.int32, device="cuda")
    score = torch.empty(R, device="cuda")
    score0 = (-torch.rand(R, generator=g) * 4 - 10).cuda()
    blen = torch.zeros(R, dtype=torch.int32, device="cuda")
    fin = torch.zeros(R, dtype=torch.int32, device="cuda")

    def ensemble(M, mode):
        def fn(i):
            L.call("fpnmt_logits_ensemble", R, V, M, (C.c_void_p * M)(*[x.data_ptr() for x in rows[:M]]),
                   (C.c_longlong * M)(*[V] * M), (C.c_float * M)(*[1.0 / M] * M), mode, fin.data_ptr(),
                   out.data_ptr(), V, L.stream_ptr())
        return fn

    def constrain(i):  # n-gram blocking, a penalty and a minimum length on the rows' history
        L.call("fpnmt_logits_constrain", R, V, work.data_ptr(), V, hist[0].data_ptr(), T + 1, t, fin.data_ptr(), 2,
               1.2, T, end, None, 0, L.stream_ptr())

    def step_log(i):
        score.copy_(score0)
        L.call("fpnmt_beam_step_log", n_img, K, V, rows[0].data_ptr(), V, score.data_ptr(), blen.data_ptr(),
               fin.data_ptr(), hist[i % 2].data_ptr(), hist[(i + 1) % 2].data_ptr(), T + 1, t, src[i % 2].data_ptr(),
               src[(i + 1) % 2].data_ptr(), T, end, tok.data_ptr(), status.data_ptr(), L.stream_ptr())

    fns = {f"ensemble_M{M}_{name}": ensemble(M, mode) for M in (2, 4) for mode, name in ((0, "prob"), (1, "logprob"))}
    fns["logits_constrain"] = constrain
    fns["beam_step_log"] = step_log
    for fn in fns.values():
        fn(0)  # loads the code object outside the capture
    torch.cuda.synchronize()
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
    assert int(fin.sum()) == 0, "beams finished: the launches did not all do the full work"
    res = {"measurement": f"logits-row launches, {R} rows x V {V}, us per launch ({launches} launches per graph, "
                          f"{replays} replays per window, {rounds} windows each, alternating; beam_step_log with its "
                          "8 KB score copy)"}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
        if name.startswith("ensemble"):
            M = int(name.split("_")[1][1:])
            nbytes = R * V * 4 * (M + 1)
            res[name]["algorithmic_bytes"] = nbytes
            res[name]["GB_per_s"] = round(nbytes / (med * 1e-6) / 1e9, 1)
    res["beam_step_log"]["read_bytes"] = R * V * 4
    print(json.dumps(res), flush=True)


def decode_bench(n_images, K, T, image, layers, V, repeats):
    import fpnmt
    from fpnmt.decode import BeamDecoder
    from fpnmt.layers import Init
    from models.transformer import Transformer
    fpnmt.set_precision("bf16")
    trs = [Transformer(layers, 512, 8, 2048, math.ceil(image / 16) ** 2, V, 0.0, max_seq_len=T,
                       init=Init(torch.Generator().manual_seed(6 + i))).cuda() for i in range(4)]
    imgs = torch.rand(n_images, image, image, 3, device="cuda") * 2 - 1
    decs = {"M1": BeamDecoder(trs[0], n_images, K, T, 2, 3, use_graph=True, mode="beam")}
    for M in (2, 4):
        for mode in ("prob", "logprob"):
            decs[f"M{M}_{mode}"] = BeamDecoder(trs[0], n_images, K, T, 2, 3, use_graph=True, mode="beam",
                                               ensemble=trs[1:M], ensemble_mode=mode)
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
    res = {"measurement": f"C5 beam decode end to end, {n_images} images x {K} beams, {layers}L, V {V}, {T} steps, "
                          f"bf16, graphs, ms per call ({repeats} calls each, alternating)"}
    one = statistics.median(times["M1"])
    for m, ts in times.items():
        med = statistics.median(ts)
        res[m] = {"median_ms": round(med, 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}
        if m != "M1":
            M = int(m[1])
            res[m]["over_M_single_decodes"] = round(med / (M * one), 3)
            res[m]["captions_other_than_M1"] = sum(a != b for a, b in zip(outs[m], outs["M1"]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", default=["kernel", "decode"], choices=["kernel", "decode"])
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--beams", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from fpnmt import _lib as L
    L.assert_in_tree()
    if "kernel" in a.what:
        kernel_bench(a.images, a.beams, a.vocab, a.steps, 5, a.launches, a.replays, a.rounds)
    if "decode" in a.what:
        decode_bench(a.images, a.beams, a.steps, 224, 6, a.vocab, a.repeats)


if __name__ == "__main__":
    main()
