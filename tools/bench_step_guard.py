"""The optimizer tail of the C2 training step of bench.py (same model, shapes,
seed and synthetic batch; imported from it, bench.py is not edited) with and
without the step guard. The tail is TrainEngine._update: fpnmt_grad_sumsq_*,
fpnmt_grad_norm_total (guard only), the AMSGrad kernel with its fused
compute-copy refresh, the step increment and the refresh of the few copies
the kernel does not write.

  off    no guard (the step as before; per-tensor clipnorm 1.0)
  guard  skip_nonfinite=True beside the per-tensor clip
  clip   clipnorm 0, global_clipnorm 1.0
  skip   guard, with an Inf in the gradient arena: every tail is skipped

One engine per setting is built and warmed up (eager call, capture, replays:
the gradient arena then holds a step's gradients), then the settings are timed
in turn, `--rounds` times over, each window `--tails` tails between two device
events; the whole step is timed the same way through graph replays (not for
`skip`, whose gradients are poisoned by hand). A tree without the guard (the
parent commit, for A/B runs of the two builds in one call) runs `off` only.
Prints one JSON line.

  python tools/bench_step_guard.py [--settings off,guard,clip,skip] [--tails 200] [--steps 100] [--rounds 3]
  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- \\
      python tools/bench_step_guard.py --tails 20 --steps 0 --rounds 1"""
import argparse
import inspect
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fpn-mt-image-captioning_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

KW = {"off": {}, "guard": dict(skip_nonfinite=True), "clip": dict(clipnorm=0.0, global_clipnorm=1.0),
      "skip": dict(skip_nonfinite=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="off,guard,clip,skip")
    ap.add_argument("--tails", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--dropout", type=float, default=0.1)
    args = ap.parse_args()

    import bench  # synthetic_batch: the benchmark's own batch
    import fpnmt
    from fpnmt.layers import Init
    from fpnmt.train import TrainEngine
    from models.transformer import Transformer
    from utils.utils import CustomSchedule
    fpnmt._lib.assert_in_tree()
    if not torch.cuda.is_available():
        raise SystemExit("bench_step_guard: needs a GPU (no fallback)")
    has_guard = "skip_nonfinite" in inspect.signature(TrainEngine.__init__).parameters
    settings = [s for s in args.settings.split(",") if s == "off" or has_guard]
    torch.cuda.set_device(0)
    fpnmt.set_precision("bf16")
    T_pad = 32
    img, tok = bench.synthetic_batch(args.batch, args.image, args.vocab, T_pad, 1000, "cuda")
    engines = {}
    for s in settings:
        model = Transformer(args.layers, 512, 8, 2048, math.ceil(args.image / 16) ** 2, args.vocab, args.dropout,
                            max_seq_len=T_pad, backbone="resnet50",
                            init=Init(torch.Generator().manual_seed(1234))).cuda()
        eng = TrainEngine(model, CustomSchedule(2048, 4000), use_graph=True, **KW[s])
        for _ in range(max(args.warmup, 3)):
            eng.step(img, tok)
        torch.cuda.synchronize()
        engines[s] = eng

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    step_ms = {s: [] for s in engines}
    tail_ms = {s: [] for s in engines}
    for _ in range(args.rounds):
        if args.steps > 0:
            for s, eng in engines.items():
                if s != "skip":
                    step_ms[s].append(window(lambda: eng.step(img, tok), args.steps))
        for s, eng in engines.items():
            if s == "skip":
                # the last segment's first element (a dense segment: the embedding, whose
                # norm the backward supplies, is not read for the total)
                eng.arena.grad[eng.arena.offsets[-1]] = float("inf")
            tail_ms[s].append(window(eng._update, args.tails))
    res = {"workload": f"C2: ResNet-50 FPN + {args.layers}-layer transformer, {args.image}x{args.image}, batch "
                       f"{args.batch}, T=31, V={args.vocab}, bf16, dropout {args.dropout}",
           "has_guard": has_guard, "tails_per_window": args.tails, "steps_per_window": args.steps,
           "rounds": args.rounds, "settings": {}}
    for s, eng in engines.items():
        ent = {"params": sum(p.numel() for p in eng.arena.params), "nblocks": eng.arena.nblocks}
        for name, ts in (("tail_ms", tail_ms[s]), ("step_ms", step_ms[s])):
            if ts:
                ent[name] = [round(t, 4) for t in ts]
                ent[name + "_median"] = round(sorted(ts)[len(ts) // 2], 4)
                ent[name + "_spread"] = round(max(ts) - min(ts), 4)
        if eng.arena.__dict__.get("guard") is not None:
            ent["guard_stats"] = {k: (v if math.isfinite(v) else str(v)) for k, v in eng.guard_stats().items()}
        res["settings"][s] = ent
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
