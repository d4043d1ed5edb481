"""A numpy restatement of the reference's per-image preprocessing (transformers 4.18 DetrFeatureExtractor with
do_resize + do_normalize on a PIL RGB image) and the collate's pad_and_create_pixel_mask.

The resize is Pillow's ImagingResample for 8-bit images with the BILINEAR filter, written as its two integer passes
over the coefficients of egtr_amd.feature_extraction.pil_bilinear_coeffs: horizontal first, then vertical, a pass
skipped when its axis keeps its size, each pass acc = 2^21 + sum_k w_k * u8 (int32 in Pillow; no overflow, so int64 here
gives the same numbers) and clip(acc >> 22, 0, 255) back to uint8.  The rescale / normalise is
(f32(u) * f32(1/255) - f32(mean_c)) / f32(std_c) in float32, as 4.18's to_numpy_array + normalize compute it."""
import numpy as np

from egtr_amd.feature_extraction import IMAGENET_MEAN, IMAGENET_STD, _target_size, pil_bilinear_coeffs

PRECISION_BITS = 22


def resample_axis(a, out_size, axis):
    """One Pillow pass along `axis` of a uint8 array."""
    in_size = a.shape[axis]
    bounds, weights = pil_bilinear_coeffs(in_size, out_size)
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    k = weights.shape[1]
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(k)[None, :], in_size - 1)   # [out, k]
    w = np.where(np.arange(k)[None, :] < bounds[:, 1:], weights, 0).astype(np.int64)
    acc = np.full((out_size,) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for j in range(k):          # taps beyond n have weight 0
        acc += w[:, j].reshape((-1,) + (1,) * (a.ndim - 1)) * a[idx[:, j]]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_resize(img, out_h, out_w):
    """PIL.Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR) for a uint8 [H, W, C] array."""
    if out_w != img.shape[1]:
        img = resample_axis(img, out_w, 1)
    if out_h != img.shape[0]:
        img = resample_axis(img, out_h, 0)
    return img


def normalize(img, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [H, W, 3] -> float32 [3, H, W], the 4.18 formula."""
    v = img.astype(np.float32) * np.float32(1 / 255.0)
    v = v.transpose(2, 0, 1)
    return (v - np.array(mean).astype(np.float32)[:, None, None]) / np.array(std).astype(np.float32)[:, None, None]


def preprocess(images, size=800, max_size=1333, do_resize=True, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Per-image resize + normalise, then the top-left zero pad and int64 mask of pad_and_create_pixel_mask."""
    outs = []
    for img in images:
        h, w = img.shape[:2]
        oh, ow = _target_size(h, w, size, max_size) if do_resize else (h, w)
        outs.append(normalize(pil_resize(img, oh, ow), mean, std))
    H = max(o.shape[1] for o in outs)
    W = max(o.shape[2] for o in outs)
    pv = np.zeros((len(outs), 3, H, W), np.float32)
    pm = np.zeros((len(outs), H, W), np.int64)
    for i, o in enumerate(outs):
        pv[i, :, :o.shape[1], :o.shape[2]] = o
        pm[i, :o.shape[1], :o.shape[2]] = 1
    return pv, pm
