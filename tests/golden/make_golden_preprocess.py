"""Writes tests/golden/preprocess.npz: what the reference's preprocessing makes of a few small seeded RGB images of
mixed sizes -- transformers 4.18 DetrFeatureExtractor (PIL BILINEAR resize, to_numpy_array's rescale by 1/255,
ImageNet normalise, all float32) followed by the collate's pad_and_create_pixel_mask.  PIL and numpy only; the
4.18 steps are restated here because transformers 4.18 itself is not required.

    python tests/golden/make_golden_preprocess.py"""
import os

import numpy as np
from PIL import Image

SIZE, MAX_SIZE = 24, 40
SHAPES = [(23, 31), (40, 17), (9, 64), (1, 5), (30, 12), (13, 13)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def get_size_with_aspect_ratio(h, w, size, max_size):
    """transformers 4.18 models/detr/feature_extraction_detr.py, on (h, w)."""
    min_original_size, max_original_size = float(min(h, w)), float(max(h, w))
    if max_original_size / min_original_size * size > max_size:
        size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def main():
    rng = np.random.default_rng(20261016)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    outs = []
    for img in images:
        oh, ow = get_size_with_aspect_ratio(img.shape[0], img.shape[1], SIZE, MAX_SIZE)
        pil = Image.fromarray(img).convert("RGB").resize((ow, oh), resample=Image.BILINEAR)
        v = np.array(pil).astype(np.float32) * (1 / 255.0)                       # to_numpy_array + rescale
        v = v.transpose(2, 0, 1)
        mean, std = np.array(MEAN).astype(v.dtype), np.array(STD).astype(v.dtype)
        outs.append((v - mean[:, None, None]) / std[:, None, None])              # normalize
    H, W = max(o.shape[1] for o in outs), max(o.shape[2] for o in outs)
    pv = np.zeros((len(outs), 3, H, W), np.float32)
    pm = np.zeros((len(outs), H, W), np.int64)
    for i, o in enumerate(outs):
        pv[i, :, :o.shape[1], :o.shape[2]] = o
        pm[i, :o.shape[1], :o.shape[2]] = 1
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preprocess.npz")
    np.savez_compressed(path, pixels=np.concatenate([x.reshape(-1) for x in images]),
                        shapes=np.array(SHAPES, np.int64), size=SIZE, max_size=MAX_SIZE,
                        pixel_values=pv, pixel_mask=pm)
    print(path, pv.shape)


if __name__ == "__main__":
    main()
