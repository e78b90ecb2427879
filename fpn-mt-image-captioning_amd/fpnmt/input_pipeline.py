"""Input pipeline: JPEG files -> the model's NHWC input batch on the GPU
(reference dataset.py:19-26 load_image and the tf.data map /
shuffle / batch / prefetch chain of dataset.py:89-92).

Split MI355X-first:
  - host: file read + JPEG decode (libjpeg through Pillow, which releases the
    GIL while decoding, so a thread pool decodes a batch in parallel; the
    reference's decode_jpeg is libjpeg too: ISLOW DCT, fancy upsampling),
    packed into ONE pinned staging buffer with an item table per batch;
  - device: one H2D copy of the packed bytes on a side stream, then ONE
    `fpnmt_image_resize_normalize` launch (bilinear resize with TF2
    half-pixel centres + mobilenet_v2.preprocess_input, bit-identical to TF's
    fp32 formula) writes the (B, S, S, 3) fp32 / bf16 input directly;
  - the next batch is decoded on the host while the current one trains
    (prefetch queue), the copy + resize of a batch is ordered before its
    consumer by a stream event (no host synchronisation);
  - optional, off by default: train-time augmentation on the device (`Augment`:
    random-resized crop, flip, brightness / contrast / saturation, one
    `fpnmt_image_aug` record per sample drawn from (seed, epoch, dataset
    index), applied by `fpnmt_image_augment_resize_normalize` in place of the
    plain launch) and a cache of decoded images by path (`DecodedCache`), so
    an image's several captions and later epochs skip the decoder while each
    pass still differs.
No CPU fallback: without the HIP library this module does not import.
"""
from __future__ import annotations

import ctypes as C
import io
import math
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import call, dtype_code

PREPROCESS_DIV = 127.5  # mobilenet_v2.preprocess_input: x / 127.5 - 1 (dataset.py:24)
PREPROCESS_SUB = 1.0
ITEM_ALIGN = 16         # byte alignment of each image inside the packed buffer


class ImageItem(C.Structure):
    """fpnmt_image_item (include/fpnmt.h)."""
    _fields_ = [("offset", C.c_longlong), ("h", C.c_int), ("w", C.c_int)]


ITEM_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])


class ImageAug(C.Structure):
    """fpnmt_image_aug (include/fpnmt.h)."""
    _fields_ = [("y0", C.c_int), ("x0", C.c_int), ("ch", C.c_int), ("cw", C.c_int), ("flip", C.c_int),
                ("brightness", C.c_float), ("contrast", C.c_float), ("saturation", C.c_float)]


AUG_DTYPE = np.dtype([("y0", "<i4"), ("x0", "<i4"), ("ch", "<i4"), ("cw", "<i4"), ("flip", "<i4"),
                      ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4")])


class AugRecord(NamedTuple):
    """One image's augmentation: the fields of fpnmt_image_aug."""
    y0: int
    x0: int
    ch: int
    cw: int
    flip: int = 0
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0


def identity_record(h, w):
    """Full box, no flip, every factor 1: fpnmt_image_resize_normalize."""
    return AugRecord(0, 0, int(h), int(w))


@dataclass(frozen=True)
class Augment:
    """Train-time augmentation settings: a random-resized crop, a left-right
    flip with probability `flip`, and brightness / contrast / saturation
    factors uniform in [1 - x, 1 + x] (0 disables the step: the factor is
    exactly 1, which the kernel skips).

    The crop follows torchvision's RandomResizedCrop: up to 10 tries of an
    area uniform in crop_scale * h * w and a log-uniform aspect ratio, then a
    centred fallback. The ratio MULTIPLIES the source's own aspect w / h (the
    reference squashes the full frame to a square, so ratio 1 at scale 1 is
    the reference's input). flip defaults to 0: captions say "left" and
    "right", and X-rays have laterality."""
    crop_scale: tuple = (0.6, 1.0)
    crop_ratio: tuple = (3 / 4, 4 / 3)
    flip: float = 0.0
    brightness: float = 0.2
    contrast: float = 0.2
    saturation: float = 0.2

    def __post_init__(self):
        s0, s1 = self.crop_scale
        r0, r1 = self.crop_ratio
        if not (0 < s0 <= s1 <= 1) or not (0 < r0 <= r1) or not math.isfinite(r1):
            raise ValueError(f"Augment: bad crop_scale {self.crop_scale} / crop_ratio {self.crop_ratio}")
        if not 0 <= self.flip <= 1:
            raise ValueError(f"Augment: flip probability {self.flip} outside [0, 1]")
        for name in ("brightness", "contrast", "saturation"):
            x = getattr(self, name)
            if not (math.isfinite(x) and x >= 0):
                raise ValueError(f"Augment: {name} {x} must be finite and >= 0")

    def draw_box(self, h, w, rng):
        """(y0, x0, ch, cw, fallback): the crop box of an (h, w) image;
        `fallback` tells that the 10 tries all missed the image."""
        h, w = int(h), int(w)
        if h <= 0 or w <= 0:
            raise ValueError(f"Augment.draw: empty image ({h}, {w})")
        area = h * w
        (s0, s1), (r0, r1) = self.crop_scale, self.crop_ratio
        for _ in range(10):
            target = area * rng.uniform(s0, s1)
            aspect = (w / h) * math.exp(rng.uniform(math.log(r0), math.log(r1)))
            cw = int(round(math.sqrt(target * aspect)))
            ch = int(round(math.sqrt(target / aspect)))
            if 0 < cw <= w and 0 < ch <= h:
                y0 = int(rng.integers(0, h - ch + 1))
                x0 = int(rng.integers(0, w - cw + 1))
                return y0, x0, ch, cw, False
        # centred fallback: the in-range ratio nearest to the whole frame (relative ratio 1)
        if r0 > 1:
            ch, cw = int(round(h / r0)), w
        elif r1 < 1:
            ch, cw = h, int(round(w * r1))
        else:
            ch, cw = h, w
        ch, cw = min(max(ch, 1), h), min(max(cw, 1), w)
        return (h - ch) // 2, (w - cw) // 2, ch, cw, True

    def _factor(self, x, rng):
        if x == 0:
            return 1.0
        return float(np.float32(rng.uniform(max(0.0, 1.0 - x), 1.0 + x)))

    def draw(self, h, w, rng) -> AugRecord:
        """One record for an (h, w) image from the numpy Generator `rng`."""
        y0, x0, ch, cw, _ = self.draw_box(h, w, rng)
        flip = int(rng.random() < self.flip) if self.flip > 0 else 0
        return AugRecord(y0, x0, ch, cw, flip, self._factor(self.brightness, rng),
                         self._factor(self.contrast, rng), self._factor(self.saturation, rng))

    @staticmethod
    def center(frac):
        """The deterministic centred box covering `frac` of each side, for
        evaluation: a function (h, w) -> record with no flip and factors 1."""
        if not 0 < frac <= 1:
            raise ValueError(f"Augment.center: frac {frac} outside (0, 1]")

        def record(h, w):
            ch = min(max(int(round(h * frac)), 1), int(h))
            cw = min(max(int(round(w * frac)), 1), int(w))
            return AugRecord((int(h) - ch) // 2, (int(w) - cw) // 2, ch, cw)
        return record


def pack_records(records, shapes, pin=False):
    """Validate records against their images' (h, w) and pack them into a
    byte tensor holding n fpnmt_image_aug structs. Returns (tensor, max_cw)."""
    n = len(records)
    if len(shapes) != n:
        raise ValueError(f"{n} records but {len(shapes)} shapes")
    buf = torch.empty(max(n, 1) * C.sizeof(ImageAug), dtype=torch.uint8, pin_memory=pin)
    rec = buf.numpy().view(AUG_DTYPE)
    rec[:] = np.zeros((), AUG_DTYPE)
    max_cw = 1
    for i, (r, (h, w)) in enumerate(zip(records, shapes)):
        r = AugRecord(*r)
        y0, x0, ch, cw = (int(v) for v in r[:4])
        if ch < 1 or cw < 1:
            raise ValueError(f"record {i}: empty box ch={ch} cw={cw}")
        if y0 < 0 or x0 < 0 or y0 + ch > h or x0 + cw > w:
            raise ValueError(f"record {i}: box ({y0}, {x0}, {ch}, {cw}) outside the ({h}, {w}) image")
        if r.flip not in (0, 1):
            raise ValueError(f"record {i}: flip {r.flip} is not 0 or 1")
        for name in ("brightness", "contrast", "saturation"):
            f = float(getattr(r, name))
            if not (math.isfinite(f) and f >= 0):
                raise ValueError(f"record {i}: {name} factor {f} must be finite and >= 0")
        rec[i] = (y0, x0, ch, cw, int(r.flip), r.brightness, r.contrast, r.saturation)
        max_cw = max(max_cw, cw)
    return buf, max_cw


def aug_records(augment, shapes, seed, epoch, indices, pin=None):
    """The batch's records: record j is drawn for the (h, w) = shapes[j] image
    from np.random.default_rng((seed, epoch, int(indices[j]))), so a sample's
    augmentation depends only on (seed, epoch, dataset index) — not on the
    batch size or composition, the thread count or the prefetch depth.
    Returns (byte tensor of n fpnmt_image_aug, max_cw); the tensor is pinned
    for the upload where there is a GPU (pin=None), or as `pin` says."""
    if pin is None:
        pin = torch.cuda.is_available()
    if len(shapes) != len(indices):
        raise ValueError(f"{len(shapes)} shapes but {len(indices)} indices")
    records = [augment.draw(h, w, np.random.default_rng((int(seed), int(epoch), int(k))))
               for (h, w), k in zip(shapes, indices)]
    return pack_records(records, [tuple(s) for s in shapes], pin=pin)


def decode_image(data: bytes) -> np.ndarray:
    """tf.image.decode_jpeg(data, channels=3) (dataset.py:22): (h, w, 3) uint8.
    Grayscale images are expanded to RGB by replication, as TF does."""
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        arr = np.asarray(im, dtype=np.uint8)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] == 0 or arr.shape[1] == 0:
        raise ValueError(f"decoded image has shape {arr.shape}, expected (h, w, 3) with h, w > 0")
    return arr


def read_image(path) -> np.ndarray:
    """tf.io.read_file + decode_jpeg(channels=3) (dataset.py:21-22)."""
    with open(path, "rb") as f:
        return decode_image(f.read())


def pack_images(images, pin=False):
    """Pack (h, w, 3) uint8 arrays into one byte buffer + an item table.
    Returns (pixels uint8 tensor, items uint8 tensor holding n
    fpnmt_image_item records, max_w)."""
    n = len(images)
    offs = np.zeros(n, dtype=np.int64)
    total = 0
    max_w = 1
    for i, im in enumerate(images):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"image {i}: expected (h, w, 3) uint8, got {im.dtype} {im.shape}")
        if im.shape[0] <= 0 or im.shape[1] <= 0:
            raise ValueError(f"image {i}: empty image {im.shape}")
        offs[i] = total
        total += -(-im.nbytes // ITEM_ALIGN) * ITEM_ALIGN
        max_w = max(max_w, im.shape[1])
    pixels = torch.empty(max(total, ITEM_ALIGN), dtype=torch.uint8, pin_memory=pin)
    flat = pixels.numpy()
    for i, im in enumerate(images):
        flat[offs[i]:offs[i] + im.nbytes] = np.ascontiguousarray(im).reshape(-1)
    items = torch.empty(max(n, 1) * C.sizeof(ImageItem), dtype=torch.uint8, pin_memory=pin)
    rec = items.numpy().view(ITEM_DTYPE)
    rec["offset"][:n] = offs
    for i, im in enumerate(images):
        rec["h"][i], rec["w"][i] = im.shape[0], im.shape[1]
    return pixels, items, max_w


def resize_normalize_packed(pixels_dev, items_dev, n, max_w, out_h, out_w, dtype=torch.float32, out=None,
                            div=PREPROCESS_DIV, sub=PREPROCESS_SUB):
    """One fpnmt_image_resize_normalize launch on the current stream over
    already-resident packed bytes -> (n, out_h, out_w, 3)."""
    dev = pixels_dev.device
    if out is None:
        out = torch.empty((n, out_h, out_w, 3), dtype=dtype, device=dev)
    if out.shape != (n, out_h, out_w, 3) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({n}, {out_h}, {out_w}, 3) tensor, got {tuple(out.shape)}")
    call("fpnmt_image_resize_normalize", items_dev.data_ptr(), n, pixels_dev.data_ptr(), pixels_dev.numel(),
         max_w, out_h, out_w, float(div), float(sub), dtype_code(out.dtype), out.data_ptr(), _lib.stream_ptr())
    return out


def resize_normalize(images, size, dtype=torch.float32, device="cuda"):
    """dataset.py:23-24 for a list of decoded (h, w, 3) uint8 images:
    (n, size, size, 3) on the GPU. `size` is an int or (out_h, out_w)."""
    out_h, out_w = (size, size) if isinstance(size, int) else size
    pixels, items, max_w = pack_images(images, pin=torch.cuda.is_available())
    pd = pixels.to(device, non_blocking=True)
    idev = items.to(device, non_blocking=True)
    out = resize_normalize_packed(pd, idev, len(images), max_w, out_h, out_w, dtype)
    return out


def load_image(img_path, caption, size, dtype=torch.float32, device="cuda"):
    """dataset.py:19-26: (image (size, size, 3) on the GPU, caption)."""
    return resize_normalize([read_image(img_path)], size, dtype, device)[0], caption


def crop_stats_packed(pixels_dev, items_dev, aug_dev, n, out=None):
    """One fpnmt_image_crop_stats call on the current stream: (n, 4) int64
    holding the R, G, B byte sums of each record's box (column 3 is 0; the
    sums stay below 2^63, so the unsigned values read as int64)."""
    if out is None:
        out = torch.empty((max(n, 1), 4), dtype=torch.int64, device=pixels_dev.device)
    if out.dtype != torch.int64 or out.numel() < 4 * n or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 tensor of >= {4 * n} elements")
    call("fpnmt_image_crop_stats", items_dev.data_ptr(), aug_dev.data_ptr(), n, pixels_dev.data_ptr(),
         pixels_dev.numel(), out.data_ptr(), _lib.stream_ptr())
    return out


def augment_resize_normalize_packed(pixels_dev, items_dev, aug_dev, n, max_cw, out_h, out_w, dtype=torch.float32,
                                    out=None, use_contrast=True, div=PREPROCESS_DIV, sub=PREPROCESS_SUB):
    """The augmented launch on the current stream over already-resident
    packed bytes, items and records -> (n, out_h, out_w, 3). With
    use_contrast the box sums are computed first (fpnmt_image_crop_stats);
    without, the contrast factors are ignored and that launch is not made."""
    dev = pixels_dev.device
    if out is None:
        out = torch.empty((n, out_h, out_w, 3), dtype=dtype, device=dev)
    if out.shape != (n, out_h, out_w, 3) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({n}, {out_h}, {out_w}, 3) tensor, got {tuple(out.shape)}")
    sums = crop_stats_packed(pixels_dev, items_dev, aug_dev, n) if use_contrast and n > 0 else None
    call("fpnmt_image_augment_resize_normalize", items_dev.data_ptr(), aug_dev.data_ptr(), _lib.ptr(sums), n,
         pixels_dev.data_ptr(), pixels_dev.numel(), max_cw, out_h, out_w, float(div), float(sub),
         dtype_code(out.dtype), out.data_ptr(), _lib.stream_ptr())
    return out


def augment_resize_normalize(images, records, size, dtype=torch.float32, device="cuda", use_contrast=True):
    """resize_normalize under one record per image (AugRecord or an 8-tuple
    in the struct's field order): (n, out_h, out_w, 3) on the GPU."""
    out_h, out_w = (size, size) if isinstance(size, int) else size
    pin = torch.cuda.is_available()
    pixels, items, _ = pack_images(images, pin=pin)
    aug, max_cw = pack_records(records, [im.shape[:2] for im in images], pin=pin)
    pd = pixels.to(device, non_blocking=True)
    idev = items.to(device, non_blocking=True)
    adev = aug.to(device, non_blocking=True)
    return augment_resize_normalize_packed(pd, idev, adev, len(images), max_cw, out_h, out_w, dtype,
                                           use_contrast=use_contrast)


class DecodedCache:
    """Decoded (h, w, 3) uint8 arrays keyed by path, for the loader's thread
    pool. The five captions of one image share one entry, and a cached sample
    skips the decoder. Once `budget` bytes are held nothing more is inserted;
    there is no eviction (the budget is meant to hold the set, or a fixed
    part of it). Two threads missing the same path both decode it, which is
    harmless: the first insert stays."""

    def __init__(self, decoder, budget):
        self.decoder = decoder
        self.budget = int(budget)
        self._lock = threading.Lock()
        self._store = {}
        self._bytes = 0
        self._hits = 0
        self._misses = 0
        self._full = False

    def __call__(self, path):
        with self._lock:
            arr = self._store.get(path)
            if arr is not None:
                self._hits += 1
                return arr
            self._misses += 1
        arr = self.decoder(path)
        with self._lock:
            if path not in self._store and not self._full:
                if self._bytes + arr.nbytes <= self.budget:
                    self._store[path] = arr
                    self._bytes += arr.nbytes
                else:
                    self._full = True  # the budget is reached: the held part stays fixed
        return arr

    def info(self):
        with self._lock:
            return {"entries": len(self._store), "bytes": self._bytes, "hits": self._hits, "misses": self._misses}


class ImageBatchLoader:
    """Batches of (images (B, S, S, 3) on the GPU, captions (B, T) int32 on the
    GPU) from image paths + padded token rows — the tf.data chain of
    dataset.py:89-92 (map(load_image) / shuffle / batch / prefetch).

    shuffle: a seeded permutation per epoch (tf.data's BUFFER_SIZE window
    shuffle is a different random order, not a numeric difference);
    drop_remainder=False keeps the short last batch like Dataset.batch.
    Decoding runs on `threads` host threads, `prefetch` batches ahead.

    augment: an Augment; each sample's record is drawn on the producer thread
    from (seed, epoch, dataset index) — epoch counting the iterations started
    before this one, as the shuffle does — and applied on the device by the
    augmented launch in place of the plain resize. cache_bytes > 0 keeps
    decoded images by path up to that many bytes (DecodedCache); the pixels
    stay uint8, so a cached image is still augmented anew every pass. With
    neither, the loader runs exactly the un-augmented path."""

    def __init__(self, paths, captions, batch_size, image_size, dtype=torch.float32, shuffle=True, seed=0,
                 threads=8, prefetch=2, device="cuda", drop_remainder=False, decoder=read_image, augment=None,
                 cache_bytes=0):
        if len(paths) != len(captions):
            raise ValueError(f"{len(paths)} paths but {len(captions)} captions")
        self.paths = list(paths)
        self.captions = np.asarray(captions, dtype=np.int32)
        self.batch_size = int(batch_size)
        self.size = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.dtype = dtype
        self.shuffle = shuffle
        self.seed = seed
        self.threads = threads
        self.prefetch = max(1, prefetch)
        self.device = torch.device(device)
        self.drop_remainder = drop_remainder
        self.decoder = decoder
        self.augment = augment
        self.cache = DecodedCache(decoder, cache_bytes) if cache_bytes > 0 else None
        self.epoch = 0

    def cache_info(self):
        """{"entries", "bytes", "hits", "misses"} of the decoded-image cache
        (all zero without one)."""
        if self.cache is None:
            return {"entries": 0, "bytes": 0, "hits": 0, "misses": 0}
        return self.cache.info()

    def __len__(self):
        n = len(self.paths)
        return n // self.batch_size if self.drop_remainder else -(-n // self.batch_size)

    def _order(self):
        idx = np.arange(len(self.paths))
        if self.shuffle:
            np.random.default_rng((self.seed, self.epoch)).shuffle(idx)
        return idx

    def _batches(self, order):
        bs = self.batch_size
        for s in range(0, len(order), bs):
            b = order[s:s + bs]
            if len(b) < bs and self.drop_remainder:
                return
            yield b

    def __iter__(self):
        order = self._order()
        epoch = self.epoch
        self.epoch += 1
        q: queue.Queue = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        pin = self.device.type == "cuda"
        decode = self.cache if self.cache is not None else self.decoder
        augment = self.augment

        def produce():
            try:
                with ThreadPoolExecutor(self.threads) as pool:
                    for b in self._batches(order):
                        if stop.is_set():
                            return
                        imgs = list(pool.map(decode, [self.paths[i] for i in b]))
                        pixels, items, max_w = pack_images(imgs, pin=pin)
                        aug = None
                        if augment is not None:
                            aug = aug_records(augment, [im.shape[:2] for im in imgs], self.seed, epoch, b, pin=pin)
                        q.put((b, pixels, items, max_w, aug))
            except BaseException as e:  # surfaced to the consumer
                q.put(e)
                return
            q.put(None)

        th = threading.Thread(target=produce, daemon=True)
        th.start()
        side = torch.cuda.Stream(self.device) if pin else None
        try:
            while True:
                got = q.get()
                if got is None:
                    break
                if isinstance(got, BaseException):
                    raise got
                b, pixels, items, max_w, aug = got
                with torch.cuda.stream(side):
                    pd = pixels.to(self.device, non_blocking=True)
                    idev = items.to(self.device, non_blocking=True)
                    caps = torch.from_numpy(self.captions[b]).to(self.device, non_blocking=True)
                    held = [pd, idev, caps]
                    if aug is None:
                        imgs = resize_normalize_packed(pd, idev, len(b), max_w, self.size[0], self.size[1], self.dtype)
                    else:
                        adev = aug[0].to(self.device, non_blocking=True)
                        # (the box sums are allocated, written and read on the side stream only)
                        imgs = augment_resize_normalize_packed(pd, idev, adev, len(b), aug[1], self.size[0],
                                                               self.size[1], self.dtype,
                                                               use_contrast=augment.contrast != 0)
                        held.append(adev)
                    held.append(imgs)
                    ev = torch.cuda.Event()
                    ev.record(side)
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                for t in held:
                    t.record_stream(cur)
                yield imgs, caps
        finally:
            stop.set()
            while th.is_alive():  # drain so the producer can exit
                try:
                    q.get_nowait()
                except queue.Empty:
                    th.join(timeout=0.05)


def default_decode_threads():
    return max(1, min(16, os.cpu_count() or 1))
