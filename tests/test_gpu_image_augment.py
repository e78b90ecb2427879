"""Train-time augmentation on the device: fpnmt_image_crop_stats and
fpnmt_image_augment_resize_normalize against the numpy restatement
(tests/image_augment_ref.py), bit for bit — the definition is a sequence of
individually rounded IEEE operations and integer sums, so every comparison is
equality — and the batch loader with augment= / cache_bytes= over JPEG files."""
import itertools

import numpy as np
import pytest
import torch

import image_augment_ref as A
from oracle import image_ref as R

pytestmark = pytest.mark.gpu

# tests/test_input_pipeline.py's ragged batch
RAGGED = [(480, 640), (1, 1), (224, 224), (100, 37), (50, 60), (333, 500), (640, 427)]


def _rng_images(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _f32(rec):
    """The record with its factors as the float32 values the struct holds."""
    return tuple(rec[:5]) + tuple(float(np.float32(v)) for v in rec[5:8])


@pytest.fixture(scope="module")
def cases():
    """[(image, record)] chosen for the places the kernels can go wrong; the
    LAST image of the batch has a box ending at its last row and column."""
    a, b, c, d, last = _rng_images([(37, 53), (100, 37), (60, 80), (480, 640), (31, 45)], seed=11)
    bright = np.random.default_rng(12).integers(150, 256, (40, 33, 3), dtype=np.uint8)
    out = [
        (a, (5, 7, 1, 1, 0, 1.0, 1.0, 1.0)),                 # a 1x1 box
        (a, (36, 52, 1, 1, 1, 1.3, 0.6, 1.7)),               # the last pixel, every step
        (a, (0, 1, 37, 52, 0, 1.0, 1.0, 1.0)),               # x0 = 1
        (a, (2, 2, 30, 40, 1, 1.0, 1.0, 1.0)),               # x0 = 2, mirrored
        (b, (9, 5, 64, 32, 0, 1.0, 1.0, 1.0)),               # x0 = 5
        (b, (3, 10, 20, 1, 1, 1.0, 1.0, 1.0)),               # cw = 1 with flip
        (b, (0, 36, 100, 1, 1, 0.8, 1.0, 0.5)),              # cw = 1 in the last column
        (c, (10, 10, 8, 6, 0, 1.0, 1.0, 1.0)),               # smaller than either output: an upscale
        (d, (0, 0, 480, 640, 0, 1.0, 1.0, 1.0)),             # much larger
        (d, (17, 101, 400, 500, 1, 1.1, 0.9, 1.2)),
        (bright, (0, 0, 40, 33, 0, 1.9, 1.0, 1.0)),          # brightness clamps at 255
        (bright, (4, 3, 30, 29, 0, 1.0, 0.0, 1.0)),          # contrast 0: the pivot everywhere
        (c, (5, 1, 50, 70, 0, 1.0, 1.8, 1.0)),               # contrast 1.8 clamps at both ends
        (c, (5, 1, 50, 70, 1, 1.0, 1.0, 1.9)),               # saturation clamps
        (c, (0, 0, 60, 80, 0, 1.0, 1.0, 0.0)),               # saturation 0: gray
    ]
    # every on / off combination of the three steps, on boxes at x0 = 1, 2, 5
    for k, (fb, fc, fs) in enumerate(itertools.product((1.0, 1.25), (1.0, 0.7), (1.0, 1.4))):
        out.append((a, (k, (1, 2, 5)[k % 3], 20 + k, 30 + k, k & 1, fb, fc, fs)))
    out.append((last, (11, 20, 20, 25, 0, 1.2, 1.15, 0.8)))  # ends at the buffer's last byte
    return [(im, _f32(r)) for im, r in out]


def _packed(images, records, exact_tail=True):
    """Device tensors of the packed batch; with exact_tail the pixel tensor
    ends at the last image's last byte (no padding up to 16 B), so the last
    rows reach the buffer's partial 16-B piece."""
    from fpnmt import input_pipeline as IP
    pixels, items, _ = IP.pack_images(images)
    aug, max_cw = IP.pack_records(records, [im.shape[:2] for im in images])
    if exact_tail:
        rec = items.numpy().view(IP.ITEM_DTYPE)
        end = int(rec["offset"][len(images) - 1]) + images[-1].nbytes
        pixels = pixels[:end]
    return pixels.cuda(), items.cuda(), aug.cuda(), max_cw


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("out_hw", [(224, 224), (64, 96)])
def test_identity_record_is_the_existing_kernel(out_hw, dtype):
    from fpnmt import input_pipeline as IP
    imgs = _rng_images(RAGGED)
    want = IP.resize_normalize(imgs, out_hw, dtype=dtype)
    got = IP.augment_resize_normalize(imgs, [IP.identity_record(*im.shape[:2]) for im in imgs], out_hw, dtype=dtype)
    assert got.dtype == dtype and torch.equal(got, want)
    assert torch.equal(IP.augment_resize_normalize(imgs, [IP.identity_record(*im.shape[:2]) for im in imgs], out_hw,
                                                   dtype=dtype, use_contrast=False), want)


@pytest.mark.parametrize("out_hw", [(224, 224), (7, 5)])
def test_augment_bit_exact(cases, out_hw):
    from fpnmt import input_pipeline as IP
    images, records = [im for im, _ in cases], [r for _, r in cases]
    assert images[-1].nbytes % 16 != 0  # the packed buffer ends in a partial 16-B piece
    pd, idev, adev, max_cw = _packed(images, records)
    assert max_cw == 640
    out = IP.augment_resize_normalize_packed(pd, idev, adev, len(images), max_cw, *out_hw).cpu().numpy()
    # a window declared narrower than the boxes: they read global memory instead
    narrow = IP.augment_resize_normalize_packed(pd, idev, adev, len(images), 4, *out_hw).cpu().numpy()
    for i, (im, rec) in enumerate(cases):
        ref = A.augment_image(im, rec, *out_hw)
        assert np.array_equal(out[i], ref), (i, rec, np.abs(out[i] - ref).max())
        assert np.array_equal(narrow[i], ref), (i, rec)


def test_augment_wide_rows():
    """A (3, 12000) image: boxes of 9000 and 11000 columns (the second is
    past the LDS window: global-memory path) and a 40-wide box, which is
    staged in LDS although its image is wide — the window follows max_cw."""
    from fpnmt import input_pipeline as IP
    wide, small = _rng_images([(3, 12000), (7, 5)], seed=5)
    for rec in [(0, 2999, 3, 9000, 0, 1.1, 0.8, 1.3), (0, 1000, 3, 11000, 1, 1.0, 1.2, 1.0),
                (1, 11950, 2, 40, 1, 0.9, 1.1, 0.6)]:
        rec = _f32(rec)
        recs = [rec, _f32((1, 1, 5, 3, 0, 1.0, 1.0, 1.0))]
        for out_hw in [(16, 224), (7, 5)]:
            out = IP.augment_resize_normalize([wide, small], recs, out_hw).cpu().numpy()
            for i, im in enumerate([wide, small]):
                assert np.array_equal(out[i], A.augment_image(im, recs[i], *out_hw)), (rec, out_hw, i)


def test_crop_stats(cases):
    from fpnmt import input_pipeline as IP
    images, records = [im for im, _ in cases], [r for _, r in cases]
    pd, idev, adev, _ = _packed(images, records)
    sums = torch.full((len(images), 4), -1, dtype=torch.int64, device="cuda")  # stale contents
    IP.crop_stats_packed(pd, idev, adev, len(images), out=sums)
    got = sums.cpu().numpy()
    for i, (im, rec) in enumerate(cases):
        assert got[i].tolist() == A.box_sums(im, rec) + [0], (i, rec)
    IP.crop_stats_packed(pd, idev, adev, len(images), out=sums)  # the zeroing belongs to the call
    assert np.array_equal(sums.cpu().numpy(), got)


def test_crop_stats_64_bit_sums():
    from fpnmt import input_pipeline as IP
    big = np.full((4200, 4100, 3), 255, np.uint8)
    pd, idev, adev, _ = _packed([big], [IP.identity_record(4200, 4100)], exact_tail=False)
    sums = IP.crop_stats_packed(pd, idev, adev, 1)
    assert 4391100000 > 2 ** 32
    assert sums.cpu().numpy()[0].tolist() == [4391100000] * 3 + [0]
    again = IP.crop_stats_packed(pd, idev, adev, 1, out=sums)
    assert again.cpu().numpy()[0].tolist() == [4391100000] * 3 + [0]


def test_null_sums_ignore_the_contrast_factor(cases):
    from fpnmt import input_pipeline as IP
    sel = [(im, r) for im, r in cases if r[6] != 1.0]
    assert len(sel) >= 6
    images, records = [im for im, _ in sel], [r for _, r in sel]
    out = IP.augment_resize_normalize(images, records, (31, 44), use_contrast=False).cpu().numpy()
    for i, (im, rec) in enumerate(sel):
        no_contrast = rec[:6] + (1.0,) + rec[7:]
        assert np.array_equal(out[i], A.augment_image(im, no_contrast, 31, 44)), (i, rec)
        assert np.array_equal(out[i], A.augment_image(im, rec, 31, 44, use_contrast=False))


def test_augment_bf16_is_rounded_fp32(cases):
    from fpnmt import input_pipeline as IP
    images, records = [im for im, _ in cases], [r for _, r in cases]
    for out_hw in [(32, 32), (7, 5)]:
        out = IP.augment_resize_normalize(images, records, out_hw, dtype=torch.bfloat16).cpu()
        assert out.dtype == torch.bfloat16
        for i, (im, rec) in enumerate(cases):
            ref = torch.from_numpy(A.augment_image(im, rec, *out_hw)).to(torch.bfloat16)
            assert torch.equal(out[i], ref), (i, rec)


def test_augment_errors_and_empty_batch():
    from fpnmt import _lib as L
    from fpnmt import input_pipeline as IP
    pd = torch.zeros(64, dtype=torch.uint8, device="cuda")
    it = torch.zeros(16, dtype=torch.uint8, device="cuda")
    au = torch.zeros(32, dtype=torch.uint8, device="cuda")
    sm = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.empty((0, 4, 4, 3), device="cuda")
    assert IP.augment_resize_normalize_packed(pd, it, au, 0, 1, 4, 4, out=out).shape == (0, 4, 4, 3)
    assert IP.crop_stats_packed(pd, it, au, 0).shape == (1, 4)
    name = "fpnmt_image_augment_resize_normalize"
    one = torch.empty((1, 4, 4, 3), device="cuda")

    def aug_call(n=1, max_cw=1, out_h=4, out_w=4, div=127.5, dtype=0, items=it, aug=au, pixels=pd, o=one, nbytes=64):
        L.call(name, L.ptr(items), L.ptr(aug), sm.data_ptr(), n, L.ptr(pixels), nbytes, max_cw, out_h, out_w, div,
               1.0, dtype, L.ptr(o), L.stream_ptr())

    for kw in (dict(out_h=0), dict(out_w=-1), dict(max_cw=0), dict(n=-1), dict(nbytes=-1)):
        with pytest.raises(RuntimeError, match="bad sizes"):
            aug_call(**kw)
    with pytest.raises(RuntimeError, match="div must be non-zero"):
        aug_call(div=0.0)
    with pytest.raises(RuntimeError, match="bad dtype"):
        aug_call(dtype=7)
    for kw in (dict(items=None), dict(aug=None), dict(pixels=None), dict(o=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            aug_call(**kw)
    with pytest.raises(RuntimeError, match="bad sizes"):
        L.call("fpnmt_image_crop_stats", it.data_ptr(), au.data_ptr(), -1, pd.data_ptr(), 64, sm.data_ptr(),
               L.stream_ptr())
    for args in ((None, au.data_ptr(), 1, pd.data_ptr(), 64, sm.data_ptr()),
                 (it.data_ptr(), None, 1, pd.data_ptr(), 64, sm.data_ptr()),
                 (it.data_ptr(), au.data_ptr(), 1, None, 64, sm.data_ptr()),
                 (it.data_ptr(), au.data_ptr(), 1, pd.data_ptr(), 64, None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            L.call("fpnmt_image_crop_stats", *args, L.stream_ptr())
    # records nobody validated: the kernels clamp the box to the image, and an
    # empty box or image writes zeros
    imgs = _rng_images([(6, 9), (5, 4)], seed=3)
    pixels, items, _ = IP.pack_images(imgs)
    raw = np.zeros(2, IP.AUG_DTYPE)
    raw[0] = (-2, 4, 100, 100, 0, 1.0, 0.5, 1.0)   # clamps to (0, 4, 6, 5)
    raw[1] = (5, 0, 3, 4, 0, 1.0, 1.0, 1.0)        # below the image: empty
    adev = torch.from_numpy(raw.view(np.uint8)).cuda()
    got = IP.augment_resize_normalize_packed(pixels.cuda(), items.cuda(), adev, 2, 100, 8, 8).cpu().numpy()
    assert np.array_equal(got[0], A.augment_image(imgs[0], (0, 4, 6, 5, 0, 1.0, 0.5, 1.0), 8, 8))
    assert (got[1] == 0).all()


# ------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def jpeg_set(tmp_path_factory):
    from PIL import Image
    from fpnmt import input_pipeline as IP
    root = tmp_path_factory.mktemp("aug_jpeg")
    shapes = [(120, 160), (64, 64), (200, 90), (31, 47), (128, 256)]
    paths = []
    for i, im in enumerate(_rng_images(shapes, seed=2)):
        p = root / f"{i}.jpg"
        Image.fromarray(im).save(p, quality=85)
        paths.append(str(p))
    return paths, [IP.read_image(p) for p in paths]


def _caps(n):
    return np.arange(n * 4, dtype=np.int32).reshape(n, 4)  # row k starts with 4k: the dataset index


def _epoch(loader):
    """{dataset index: image tensor on the host} of one pass."""
    got = {}
    for images, c in loader:
        torch.cuda.synchronize()
        for j in range(images.shape[0]):
            k = int(c[j, 0].item()) // 4
            assert k not in got
            got[k] = images[j].cpu()
    return got


def test_loader_augments_per_seed_epoch_index(jpeg_set):
    from fpnmt import input_pipeline as IP
    paths, decoded = jpeg_set
    aug = IP.Augment(flip=0.5)

    def loader(batch_size, threads):
        return IP.ImageBatchLoader(paths, _caps(len(paths)), batch_size=batch_size, image_size=96, shuffle=True,
                                   seed=3, threads=threads, augment=aug)

    ld = loader(2, 3)
    epochs = [_epoch(ld), _epoch(ld)]
    for epoch, got in enumerate(epochs):
        assert sorted(got) == list(range(len(paths)))
        for k, im in enumerate(decoded):
            buf, _ = IP.aug_records(aug, [im.shape[:2]], 3, epoch, [k])
            rec = tuple(buf.numpy().view(IP.AUG_DTYPE)[0].tolist())
            assert np.array_equal(got[k].numpy(), A.augment_image(im, rec, 96, 96)), (epoch, k, rec)
    assert any(not torch.equal(epochs[0][k], epochs[1][k]) for k in epochs[0])
    other = loader(3, 1)
    for want in epochs:  # another batch size and thread count: the same tensors per dataset index
        got = _epoch(other)
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_loader_cache_decodes_each_path_once(jpeg_set):
    from fpnmt import input_pipeline as IP
    paths, decoded = jpeg_set
    twice = paths + paths
    count = {}

    def decoder(path):
        count[path] = count.get(path, 0) + 1
        return IP.read_image(path)

    aug = IP.Augment()
    # (one decode thread: two threads missing the same path at once would both decode it)
    cached = IP.ImageBatchLoader(twice, _caps(len(twice)), batch_size=4, image_size=64, seed=5, threads=1,
                                 decoder=decoder, augment=aug, cache_bytes=1 << 24)
    plain = IP.ImageBatchLoader(twice, _caps(len(twice)), batch_size=4, image_size=64, seed=5, threads=2, augment=aug)
    for _ in range(2):
        got, want = _epoch(cached), _epoch(plain)
        assert sorted(got) == list(range(len(twice)))
        assert all(torch.equal(got[k], want[k]) for k in want)
    assert count == {p: 1 for p in paths}
    assert cached.cache_info() == {"entries": len(paths), "bytes": sum(im.nbytes for im in decoded),
                                   "hits": 2 * len(twice) - len(paths), "misses": len(paths)}
    assert plain.cache_info()["entries"] == 0


def test_loader_defaults_are_the_plain_path(jpeg_set):
    from fpnmt import input_pipeline as IP
    paths, decoded = jpeg_set
    got = _epoch(IP.ImageBatchLoader(paths, _caps(len(paths)), batch_size=2, image_size=96, seed=3, threads=2,
                                     augment=None, cache_bytes=0))
    for k, im in enumerate(decoded):
        assert np.array_equal(got[k].numpy(), R.load_image_pixels(im, 96))
