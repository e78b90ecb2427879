"""The augmented image path (include/fpnmt.h: fpnmt_image_aug) restated in
numpy float32 on top of oracle/image_ref.py, for the augmentation tests.

A record is (y0, x0, ch, cw, flip, brightness, contrast, saturation). The
output is the TF2 bilinear resize of the box (mirrored if flip), then on the
resized fp32 value in [0, 255], each step clamped to [0, 255] and skipped
when its factor is exactly 1:
  contrast   v = m + (v - m) * c, m = the mean luma of the SOURCE box from
             its integer byte sums: G = 299 S_R + 587 S_G + 114 S_B in Python
             integers, m = float32(float64(G) / float64(1000 ch cw));
  brightness v = v * b;
  saturation g = 0.299f r + 0.587f g + 0.114f b (left to right),
             v = g + (v - g) * s;
then preprocess_input. numpy float32 array arithmetic rounds every multiply
and add separately, which is the definition.
"""
import numpy as np

from oracle import image_ref as R

F32 = np.float32


def box_sums(img_u8, rec):
    """R, G, B byte sums of the record's box, as Python integers."""
    y0, x0, ch, cw = (int(v) for v in rec[:4])
    s = img_u8[y0:y0 + ch, x0:x0 + cw].reshape(-1, 3).sum(0, dtype=np.uint64)
    return [int(v) for v in s]


def box_mean_luma(img_u8, rec):
    ch, cw = int(rec[2]), int(rec[3])
    sr, sg, sb = box_sums(img_u8, rec)
    G = 299 * sr + 587 * sg + 114 * sb
    return F32(np.float64(G) / np.float64(1000 * ch * cw))


def _clamp(v):
    return np.clip(v, F32(0), F32(255)).astype(F32)


def augment_pixels(img_u8, rec, out_h, out_w, use_contrast=True):
    """The resized, colour-adjusted fp32 values in [0, 255] (before the
    normalisation): (out_h, out_w, 3)."""
    y0, x0, ch, cw, flip = (int(v) for v in rec[:5])
    b, c, s = (F32(v) for v in rec[5:8])
    box = img_u8[y0:y0 + ch, x0:x0 + cw]
    if flip:
        box = box[:, ::-1]
    v = R.resize_bilinear(box, out_h, out_w)
    if use_contrast and c != F32(1):
        m = box_mean_luma(img_u8, rec)
        v = _clamp(m + (v - m) * c)
    if b != F32(1):
        v = _clamp(v * b)
    if s != F32(1):
        g = F32(0.299) * v[..., 0] + F32(0.587) * v[..., 1] + F32(0.114) * v[..., 2]
        g = g[..., None]
        v = _clamp(g + (v - g) * s)
    return v.astype(F32)


def augment_image(img_u8, rec, out_h, out_w, use_contrast=True):
    """What fpnmt_image_augment_resize_normalize writes for one image (fp32)."""
    return R.preprocess_input(augment_pixels(img_u8, rec, out_h, out_w, use_contrast))
