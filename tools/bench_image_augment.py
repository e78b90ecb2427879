"""Train-time augmentation and the decoded-image cache, measured.

  kernel: 256 resident decoded 480 x 640 images -> (256, 224, 224, 3) fp32
          (bench.py's input_pipeline_probe shape), HIP events around windows
          of `--launches` launches, the four variants alternating for
          `--rounds` rounds after a warm-up of each:
            plain     fpnmt_image_resize_normalize (untouched: the baseline)
            identity  fpnmt_image_augment_resize_normalize, identity records,
                      no box sums
            augment   fpnmt_image_crop_stats + the augmented launch under
                      default-Augment records
            stats     fpnmt_image_crop_stats alone under the same records
                      (its zero fill included)
          Prints every window, the medians, each variant's own spread
          (max - min of its windows) and the algorithmic bytes per call.
  loader: `--files` synthetic 480 x 640 JPEG files in a temporary directory,
          every path listed five times (one sample per caption), default
          Augment, `--threads` decode threads: images/s of a whole pass with
          cache_bytes=0 and of the SECOND pass of a loader whose cache holds
          the set (host clock around a pass that ends in a device
          synchronise).

Prints one JSON line per measurement. Run from the repository root:
  python tools/bench_image_augment.py [kernel] [loader]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fpn-mt-image-captioning_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def _images(n, src, seed=7):
    base = np.random.default_rng(seed).integers(0, 256, (src[0], src[1], 3), dtype=np.uint8)
    return [np.roll(base, i, axis=1) for i in range(n)]


def kernel_bench(a):
    from fpnmt import input_pipeline as IP
    n, src, size = a.images, (480, 640), 224
    imgs = _images(n, src)
    shapes = [im.shape[:2] for im in imgs]
    pixels, items, max_w = IP.pack_images(imgs, pin=True)
    ident, ident_cw = IP.pack_records([IP.identity_record(*s) for s in shapes], shapes, pin=True)
    drawn, drawn_cw = IP.aug_records(IP.Augment(), shapes, 0, 0, range(n), pin=True)
    pd, idev, iddev, drdev = pixels.cuda(), items.cuda(), ident.cuda(), drawn.cuda()
    out = torch.empty((n, size, size, 3), device="cuda")
    sums = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    rec = drawn.numpy().view(IP.AUG_DTYPE)[:n]
    box_bytes = int((rec["ch"].astype(np.int64) * rec["cw"] * 3).sum())
    src_bytes, out_bytes = n * src[0] * src[1] * 3, out.numel() * 4

    def plain():
        IP.resize_normalize_packed(pd, idev, n, max_w, size, size, out=out)

    def identity():
        IP.augment_resize_normalize_packed(pd, idev, iddev, n, ident_cw, size, size, out=out, use_contrast=False)

    def augment():
        # (crop_stats_packed + the launch, with the sums buffer held, as the loader's call does per batch)
        IP.crop_stats_packed(pd, idev, drdev, n, out=sums)
        IP.call("fpnmt_image_augment_resize_normalize", idev.data_ptr(), drdev.data_ptr(), sums.data_ptr(), n,
                pd.data_ptr(), pd.numel(), drawn_cw, size, size, IP.PREPROCESS_DIV, IP.PREPROCESS_SUB,
                IP.dtype_code(out.dtype), out.data_ptr(), IP._lib.stream_ptr())

    def stats():
        IP.crop_stats_packed(pd, idev, drdev, n, out=sums)

    variants = {"plain": plain, "identity": identity, "augment": augment, "stats": stats}
    # algorithmic bytes: every needed source byte once + the fp32 output; the
    # augmented call reads its boxes twice (sums, then the resize)
    need = {"plain": src_bytes + out_bytes, "identity": src_bytes + out_bytes, "augment": 2 * box_bytes + out_bytes,
            "stats": box_bytes}
    st = torch.cuda.current_stream()
    for f in variants.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    windows = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.launches):
                f()
            e1.record(st)
            torch.cuda.synchronize()
            windows[k].append(e0.elapsed_time(e1) / a.launches)
    res = {"bench": "kernel", "workload": f"{n} decoded {src[0]}x{src[1]} RGB images -> ({n}, {size}, {size}, 3) fp32",
           "launches_per_window": a.launches, "rounds": a.rounds,
           "augment_box_fraction_of_source": round(box_bytes / src_bytes, 4)}
    base = statistics.median(windows["plain"])
    for k, w in windows.items():
        ms = statistics.median(w)
        res[k] = {"ms": round(ms, 4), "windows_ms": [round(x, 4) for x in w], "spread_ms": round(max(w) - min(w), 4),
                  "vs_plain": round(ms / base, 3), "algorithmic_bytes": need[k],
                  "algorithmic_gb_per_s": round(need[k] / (ms * 1e-3) / 1e9, 1),
                  "frac_of_hbm_peak": round(need[k] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    print(json.dumps(res), flush=True)


def loader_bench(a):
    from PIL import Image
    from fpnmt import input_pipeline as IP
    imgs = _images(a.files, (480, 640), seed=9)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, im in enumerate(imgs):
            p = os.path.join(d, f"{i}.jpg")
            Image.fromarray(im).save(p, quality=90)
            paths.append(p)
        listed = paths * 5  # one sample per caption
        caps = np.zeros((len(listed), 4), np.int32)
        set_bytes = sum(im.nbytes for im in imgs)

        def one_pass(loader):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seen = 0
            for images, _ in loader:
                seen += images.shape[0]
            torch.cuda.synchronize()
            return seen / (time.perf_counter() - t0)

        def make(cache_bytes):
            return IP.ImageBatchLoader(listed, caps, batch_size=a.batch, image_size=224, seed=1, threads=a.threads,
                                       augment=IP.Augment(), cache_bytes=cache_bytes)

        one_pass(IP.ImageBatchLoader(listed[:4 * a.batch], caps[:4 * a.batch], batch_size=a.batch, image_size=224,
                                     threads=a.threads, augment=IP.Augment()))  # warm-up: code objects, the pool
        plain, cached = make(0), make(2 * set_bytes)
        rates = {"uncached": [], "cached_first_pass": [], "cached_later_pass": []}
        rates["cached_first_pass"].append(one_pass(cached))
        for _ in range(a.passes):  # alternating, so both see the same neighbours on the host
            rates["uncached"].append(one_pass(plain))
            rates["cached_later_pass"].append(one_pass(cached))
        print(json.dumps({
            "bench": "loader", "files": a.files, "samples_per_pass": len(listed), "threads": a.threads,
            "batch": a.batch, "jpeg": "480x640 q90 (random pixels), Pillow (libjpeg)",
            "cache": cached.cache_info(), "set_bytes": set_bytes,
            "images_per_s": {k: {"median": round(statistics.median(v), 1), "passes": [round(x, 1) for x in v]}
                             for k, v in rates.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="*", help="kernel and / or loader (default: both)")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--files", type=int, default=300)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    what = a.what or ["kernel", "loader"]
    if set(what) - {"kernel", "loader"}:
        ap.error(f"unknown measurement in {what}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_augment: no GPU (there is no CPU path to measure)")
    from fpnmt import _lib
    _lib.assert_in_tree()
    for w in what:
        {"kernel": kernel_bench, "loader": loader_bench}[w](a)


if __name__ == "__main__":
    main()
