"""Train-time augmentation, host side (no GPU): Augment.draw's boxes and
factors, the per-sample determinism and struct layout of aug_records, record
validation, the decoded-image cache, and known answers of the numpy
restatement (tests/image_augment_ref.py) the GPU tests compare against."""
import ctypes
import threading

import numpy as np
import pytest

import image_augment_ref as A
from oracle import image_ref as R

SHAPES = [(1, 1), (1, 37), (37, 1), (2, 3), (100, 37), (480, 640), (640, 427)]
SEEDS = 200


def _check_box(rec, h, w):
    y0, x0, ch, cw = rec[:4]
    assert all(isinstance(v, int) for v in rec[:5])
    assert ch >= 1 and cw >= 1
    assert 0 <= y0 and y0 + ch <= h and 0 <= x0 and x0 + cw <= w


def test_draw_boxes_and_factors():
    from fpnmt import input_pipeline as IP
    aug = IP.Augment()
    s0, s1 = aug.crop_scale
    fallbacks = {}
    for h, w in SHAPES:
        n_fb = 0
        for seed in range(SEEDS):
            y0, x0, ch, cw, fb = aug.draw_box(h, w, np.random.default_rng(seed))
            rec = aug.draw(h, w, np.random.default_rng(seed))
            assert rec[:4] == (y0, x0, ch, cw)  # draw() is draw_box() + the factors
            _check_box(rec, h, w)
            n_fb += fb
            if not fb:
                # ch and cw are each the exact side rounded to the nearest
                # integer, so the exact area s*h*w lies between the areas of
                # the boxes half a pixel smaller and larger on both sides
                assert (ch + 0.5) * (cw + 0.5) >= s0 * h * w
                assert max(ch - 0.5, 0) * max(cw - 0.5, 0) <= s1 * h * w
            assert rec.flip == 0  # the default probability is 0
            for f, x in ((rec.brightness, aug.brightness), (rec.contrast, aug.contrast),
                         (rec.saturation, aug.saturation)):
                # float32 rounding is monotonic: the rounded draw lies between the rounded ends
                assert np.float32(1 - x) <= np.float32(f) <= np.float32(1 + x)
                assert np.float32(f) == f  # already a float32 value: packing does not change it
        fallbacks[(h, w)] = n_fb
    # observed with the default settings: 0 fallbacks in 200 draws for every
    # shape of SHAPES, (480, 640) included (a try misses with probability
    # ~0.3, ten in a row with ~1e-5); the cap is 5 % of 200
    assert fallbacks[(480, 640)] <= 10, fallbacks


def test_disabled_colour_steps_are_exactly_one_and_flip_probability():
    from fpnmt import input_pipeline as IP
    aug = IP.Augment(brightness=0, contrast=0.3, saturation=0)
    recs = [aug.draw(50, 60, np.random.default_rng(s)) for s in range(50)]
    assert all(r.brightness == 1.0 and r.saturation == 1.0 for r in recs)
    assert any(r.contrast != 1.0 for r in recs)
    always = IP.Augment(flip=1.0)
    assert all(always.draw(9, 9, np.random.default_rng(s)).flip == 1 for s in range(20))
    half = IP.Augment(flip=0.5)
    flips = sum(half.draw(9, 9, np.random.default_rng(s)).flip for s in range(200))
    assert 60 <= flips <= 140  # 100 +- 5.7 sigma of a fair coin
    with pytest.raises(ValueError):
        IP.Augment(brightness=-0.1)
    with pytest.raises(ValueError):
        IP.Augment(crop_scale=(0.0, 1.0))


def test_identity_settings_draw_the_identity_record():
    from fpnmt import input_pipeline as IP
    aug = IP.Augment(crop_scale=(1, 1), crop_ratio=(1, 1), flip=0, brightness=0, contrast=0, saturation=0)
    for h, w in SHAPES:
        for seed in range(5):
            rec = aug.draw(h, w, np.random.default_rng(seed))
            assert rec == IP.identity_record(h, w) == (0, 0, h, w, 0, 1.0, 1.0, 1.0)


def test_fallback_is_the_centred_box():
    from fpnmt import input_pipeline as IP
    # ratios all above the frame's: no try can fit at scale 1, the fallback keeps the width
    aug = IP.Augment(crop_scale=(1, 1), crop_ratio=(2, 3))
    y0, x0, ch, cw, fb = aug.draw_box(100, 80, np.random.default_rng(0))
    assert fb and (y0, x0, ch, cw) == (25, 0, 50, 80)
    aug = IP.Augment(crop_scale=(1, 1), crop_ratio=(0.25, 0.5))
    y0, x0, ch, cw, fb = aug.draw_box(100, 80, np.random.default_rng(0))
    assert fb and (y0, x0, ch, cw) == (0, 20, 100, 40)
    assert IP.Augment.center(0.5)(100, 80) == (25, 20, 50, 40, 0, 1.0, 1.0, 1.0)
    assert IP.Augment.center(1.0)(1, 1) == IP.identity_record(1, 1)
    assert IP.Augment.center(0.1)(1, 3)[:4] == (0, 1, 1, 1)


def test_aug_records_depend_on_seed_epoch_index_only():
    from fpnmt import input_pipeline as IP
    aug = IP.Augment(flip=0.5)
    shape_of = {k: (40 + 3 * k, 50 + 7 * k) for k in range(10)}

    def rows(indices, seed=7, epoch=2):
        buf, max_cw = IP.aug_records(aug, [shape_of[k] for k in indices], seed, epoch, indices)
        raw = buf.numpy().reshape(-1, 32)
        assert raw.shape[0] == len(indices)
        assert max_cw == int(raw.view(IP.AUG_DTYPE)["cw"].max())
        return {k: raw[j].tobytes() for j, k in enumerate(indices)}

    a = rows([3, 1, 4])
    b = rows(np.array([9, 4, 0, 3, 2, 1, 5], dtype=np.int64))
    for k in (1, 3, 4):
        assert a[k] == b[k]
    assert rows([3, 1, 4]) == a
    other = rows([3, 1, 4], epoch=3)
    assert all(other[k] != a[k] for k in (1, 3, 4))
    assert rows([3], seed=8)[3] != a[3]
    # the packed record is what draw gives under that generator
    rec = aug.draw(*shape_of[4], np.random.default_rng((7, 2, 4)))
    got = np.frombuffer(a[4], dtype=IP.AUG_DTYPE)[0]
    assert tuple(got.tolist()) == tuple(rec)


def test_aug_struct_layout():
    from fpnmt import input_pipeline as IP
    assert ctypes.sizeof(IP.ImageAug) == IP.AUG_DTYPE.itemsize == 32
    names = ["y0", "x0", "ch", "cw", "flip", "brightness", "contrast", "saturation"]
    assert [f[0] for f in IP.ImageAug._fields_] == names == list(IP.AUG_DTYPE.names) == list(IP.AugRecord._fields)
    for i, name in enumerate(names):
        assert getattr(IP.ImageAug, name).offset == 4 * i == IP.AUG_DTYPE.fields[name][1]
    buf, max_cw = IP.pack_records([(1, 2, 3, 4, 1, 0.5, 1.25, 2.0)], [(10, 10)])
    s = IP.ImageAug.from_buffer_copy(buf.numpy().tobytes())
    assert (s.y0, s.x0, s.ch, s.cw, s.flip, s.brightness, s.contrast, s.saturation) == (1, 2, 3, 4, 1, 0.5, 1.25, 2.0)
    assert max_cw == 4


@pytest.mark.parametrize("rec, what", [
    ((0, 0, 5, 11, 0, 1, 1, 1), "outside"),
    ((3, 0, 8, 4, 0, 1, 1, 1), "outside"),
    ((-1, 0, 4, 4, 0, 1, 1, 1), "outside"),
    ((0, 0, 4, 0, 0, 1, 1, 1), "empty box"),
    ((0, 0, 0, 4, 0, 1, 1, 1), "empty box"),
    ((0, 0, 4, 4, 0, float("nan"), 1, 1), "brightness"),
    ((0, 0, 4, 4, 0, 1, float("inf"), 1), "contrast"),
    ((0, 0, 4, 4, 0, 1, 1, -0.5), "saturation"),
    ((0, 0, 4, 4, 2, 1, 1, 1), "flip"),
])
def test_record_validation(rec, what):
    from fpnmt import input_pipeline as IP
    with pytest.raises(ValueError, match=what):
        IP.pack_records([rec], [(10, 10)])


def test_decoded_cache_counts_and_budget():
    from fpnmt import input_pipeline as IP
    calls = []
    lock = threading.Lock()

    def decoder(path):
        with lock:
            calls.append(path)
        return np.full((4, 5, 3), int(path[1:]), np.uint8)  # 60 bytes each

    cache = IP.DecodedCache(decoder, budget=150)  # room for two images
    paths = ["p0", "p1", "p0", "p2", "p1", "p2", "p3", "p0"]
    for p in paths:
        arr = cache(p)
        assert arr.shape == (4, 5, 3) and int(arr[0, 0, 0]) == int(p[1:])
    # p0 and p1 are held; p2 did not fit, which closed the cache; p2 and p3 decode every time
    assert calls == ["p0", "p1", "p2", "p2", "p3"]
    assert cache.info() == {"entries": 2, "bytes": 120, "hits": 3, "misses": 5}

    calls.clear()
    big = IP.DecodedCache(decoder, budget=1 << 20)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:
        for _ in range(3):
            list(pool.map(big, ["p0", "p1", "p2", "p3", "p4"]))
    assert sorted(calls) == ["p0", "p1", "p2", "p3", "p4"]  # distinct paths within a map: one decode each
    assert big.info() == {"entries": 5, "bytes": 300, "hits": 10, "misses": 5}


def test_loader_builds_its_cache_without_a_device():
    from fpnmt import input_pipeline as IP
    caps = np.zeros((4, 3), np.int32)
    plain = IP.ImageBatchLoader(["a", "b", "a", "b"], caps, 2, 8, device="cpu")
    assert plain.cache is None and plain.augment is None
    assert plain.cache_info() == {"entries": 0, "bytes": 0, "hits": 0, "misses": 0}
    n = [0]

    def decoder(path):
        n[0] += 1
        return np.zeros((2, 2, 3), np.uint8)

    ld = IP.ImageBatchLoader(["a", "b", "a", "b"], caps, 2, 8, device="cpu", decoder=decoder, cache_bytes=100,
                             augment=IP.Augment())
    for p in ld.paths:
        ld.cache(p)
    assert n[0] == 2 and ld.cache_info() == {"entries": 2, "bytes": 24, "hits": 2, "misses": 2}


# ------------------------------------------------------------ restatement KATs
def _img(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_ref_identity_is_load_image_pixels():
    img = _img(23, 31)
    out = A.augment_image(img, (0, 0, 23, 31, 0, 1.0, 1.0, 1.0), 16, 16)
    assert out.dtype == np.float32 and np.array_equal(out, R.load_image_pixels(img, 16))


def test_ref_saturation_zero_is_gray():
    img = _img(9, 7, 1)
    v = A.augment_pixels(img, (1, 2, 6, 4, 0, 1.0, 1.0, 0.0), 5, 6)
    assert np.array_equal(v[..., 0], v[..., 1]) and np.array_equal(v[..., 1], v[..., 2])
    plain = A.augment_pixels(img, (1, 2, 6, 4, 0, 1.0, 1.0, 1.0), 5, 6)
    g = np.float32(0.299) * plain[..., 0] + np.float32(0.587) * plain[..., 1] + np.float32(0.114) * plain[..., 2]
    assert np.array_equal(v[..., 0], g)


def test_ref_contrast_zero_is_the_box_mean_luma():
    img = np.zeros((4, 4, 3), np.uint8)
    img[1:3, 1:3] = [[[10, 20, 30], [50, 60, 70]], [[90, 100, 110], [130, 140, 150]]]
    rec = (1, 1, 2, 2, 0, 1.0, 0.0, 1.0)
    assert A.box_sums(img, rec) == [280, 320, 360]
    m = A.box_mean_luma(img, rec)
    # (299*280 + 587*320 + 114*360) / 4000 = 312600 / 4000
    assert m == np.float32(78.15)
    v = A.augment_pixels(img, rec, 3, 5)
    assert (v == m).all()
    assert np.array_equal(A.augment_pixels(img, rec, 3, 5, use_contrast=False),
                          A.augment_pixels(img, (1, 1, 2, 2, 0, 1.0, 1.0, 1.0), 3, 5))


def test_ref_flip_and_clamp():
    img = _img(6, 8, 2)
    a = A.augment_pixels(img, (0, 2, 6, 5, 1, 1.0, 1.0, 1.0), 6, 5)
    assert np.array_equal(a, img[:, 2:7][:, ::-1].astype(np.float32))  # identity size: the mirrored box
    bright = A.augment_pixels(np.full((3, 3, 3), 200, np.uint8), (0, 0, 3, 3, 0, 1.9, 1.0, 1.0), 2, 2)
    assert (bright == 255).all()
