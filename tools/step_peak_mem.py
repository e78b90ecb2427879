"""Peak allocated device memory of the C2 training step (bench.py's model,
batch and graph replay): python tools/step_peak_mem.py [defer_conv_wgrads]
(0 / 1 / a class mask; default: the shipped config). Prints one JSON line."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fpn-mt-image-captioning_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fpnmt  # noqa: E402
from bench import synthetic_batch  # noqa: E402
from fpnmt.layers import Init  # noqa: E402
from fpnmt.train import TrainEngine  # noqa: E402
from models.transformer import Transformer  # noqa: E402
from utils.utils import CustomSchedule  # noqa: E402

if len(sys.argv) > 1:
    v = int(sys.argv[1])
    fpnmt.config.defer_conv_wgrads = bool(v) if v in (0, 1) else v
torch.cuda.set_device(0)
fpnmt.set_precision("bf16")
model = Transformer(6, 512, 8, 2048, math.ceil(224 / 16) ** 2, 10000, 0.1, max_seq_len=32, backbone="resnet50",
                    init=Init(torch.Generator().manual_seed(1234))).cuda()
eng = TrainEngine(model, CustomSchedule(2048, 4000), use_graph=True)
img, tok = synthetic_batch(32, 224, 10000, 32, 1000, "cuda")
for _ in range(5):
    loss = eng.step(img, tok)
torch.cuda.synchronize()
print(json.dumps({"defer_conv_wgrads": fpnmt.config.defer_conv_wgrads, "loss": float(loss),
                  "peak_allocated_MiB": round(torch.cuda.max_memory_allocated() / 2**20, 1),
                  "peak_reserved_MiB": round(torch.cuda.max_memory_reserved() / 2**20, 1)}))
