"""The C2 training step of bench.py (same model, shapes, seed and synthetic
batch; imported from it, bench.py is not edited) with and without weight
averaging:

  a  no average (ema_decay=None: the plain step)
  b  ema_decay=0.999 (fpnmt_amsgrad_step_ema: one more fp32 stream in the
     optimizer kernel, 8 B per trainable parameter per step)
  c  b with the backbone frozen

One engine per setting is built and warmed up (eager call, capture, replays),
then the settings are timed in turn, `--rounds` times over, each window
`--steps` graph replays between two device events (>= 1 s at the default):
the spread of a setting over the rounds is printed next to the differences
between settings. Prints one JSON line.

  python tools/bench_ema.py [--settings abc] [--steps 150] [--rounds 3]
  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- \\
      python tools/bench_ema.py --settings b --steps 20 --rounds 1
(the kernel trace then has amsgrad_kernel<PREP, GROUPS, EMA>'s own time; its
bytes are 36 B per trainable parameter without the average and 44 B with it,
plus 4 B per bf16 compute-copy element written by the fused refresh)."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fpn-mt-image-captioning_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

DECAY = 0.999


def engine_kw(setting, model):
    from fpnmt import param_groups as G
    if setting == "a":
        return {}
    if setting == "b":
        return dict(ema_decay=DECAY)
    if setting == "c":
        return dict(ema_decay=DECAY, param_groups=[G.backbone_group(model, frozen=True)])
    raise ValueError(setting)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="abc")
    ap.add_argument("--steps", type=int, default=150)
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
        raise SystemExit("bench_ema: needs a GPU (no fallback)")
    torch.cuda.set_device(0)
    fpnmt.set_precision("bf16")
    T_pad = 32
    img, tok = bench.synthetic_batch(args.batch, args.image, args.vocab, T_pad, 1000, "cuda")
    engines = {}
    for s in args.settings:
        model = Transformer(args.layers, 512, 8, 2048, math.ceil(args.image / 16) ** 2, args.vocab, args.dropout,
                            max_seq_len=T_pad, backbone="resnet50",
                            init=Init(torch.Generator().manual_seed(1234))).cuda()
        eng = TrainEngine(model, CustomSchedule(2048, 4000), use_graph=True, **engine_kw(s, model))
        for _ in range(max(args.warmup, 3)):
            eng.step(img, tok)
        torch.cuda.synchronize()
        engines[s] = eng
    times = {s: [] for s in engines}
    loss = {}
    for _ in range(args.rounds):
        for s, eng in engines.items():
            eng.step(img, tok)  # this engine's graphs and weights back into the caches
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                out = eng.step(img, tok)
            e1.record()
            torch.cuda.synchronize()
            times[s].append(e0.elapsed_time(e1) / args.steps)
            loss[s] = float(out)
    res = {"workload": f"C2: ResNet-50 FPN + {args.layers}-layer transformer, {args.image}x{args.image}, batch "
                       f"{args.batch}, T=31, V={args.vocab}, bf16, dropout {args.dropout}, hipGraph replay",
           "ema_decay": DECAY, "steps_per_window": args.steps, "rounds": args.rounds, "settings": {}}
    for s, ts in times.items():
        med = sorted(ts)[len(ts) // 2]
        a = engines[s].arena
        sg = engines[s].seg_groups
        live = sum(p.numel() for i, p in enumerate(a.params) if sg is None or not sg.frozen[i])
        res["settings"][s] = {"ms_per_step": [round(t, 4) for t in ts], "median_ms": round(med, 4),
                              "spread_ms": round(max(ts) - min(ts), 4), "window_s": round(med * args.steps / 1e3, 3),
                              "images_per_s": round(args.batch / med * 1e3, 1), "loss": round(loss[s], 5),
                              "updated_params": live,
                              "optimizer_stream_bytes": live * (44 if a.ema is not None else 36)}
    if "a" in times:
        base = res["settings"]["a"]["median_ms"]
        for s in times:
            res["settings"][s]["vs_a"] = round(res["settings"][s]["median_ms"] / base, 4)
            res["settings"][s]["minus_a_ms"] = round(res["settings"][s]["median_ms"] - base, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
