"""CPU: the reference-exact preprocessing of DeformableDetrDeviceFeatureExtractor, checked on the host --
pil_bilinear_coeffs plus the restated integer passes (tests/pil_resample_restated.py) against Pillow's own resize, the
normalisation table against the transformers 4.18 float32 formula, output sizes and labels against the existing
extractor, and the committed golden (tests/golden/make_golden_preprocess.py) against the restatement."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pil_resample_restated as R  # noqa: E402

from egtr_amd import feature_extraction as FE  # noqa: E402
from egtr_amd.feature_extraction import (DeformableDetrDeviceFeatureExtractor, DeformableDetrFeatureExtractor,  # noqa: E402
                                         _target_size, normalize_lut, pil_bilinear_coeffs)


def size_pairs():
    """>= 200 seeded (h, w, out_h, out_w): up to 8x up, down to 1/8, one axis unchanged, 1-pixel ends, odd sizes and
    the VG-like shapes of size=800 / max_size=1333 (and 600 / 1000)."""
    rng = np.random.default_rng(7)
    pairs = []
    for _ in range(60):                                   # free ratios in [1/8, 8]
        h, w = (int(v) for v in rng.integers(1, 120, 2))
        fh, fw = np.exp(rng.uniform(np.log(1 / 8), np.log(8), 2))
        pairs.append((h, w, max(1, int(h * fh)), max(1, int(w * fw))))
    for _ in range(30):                                   # one axis unchanged
        h, w = (int(v) for v in rng.integers(1, 150, 2))
        o = int(rng.integers(1, 300))
        pairs.append((h, w, h, o) if rng.random() < 0.5 else (h, w, o, w))
    for _ in range(30):                                   # 1-pixel inputs / outputs
        n = int(rng.integers(1, 200))
        pairs += [(1, n, int(rng.integers(1, 40)), int(rng.integers(1, 300))), (n, 1, int(rng.integers(1, 300)), 1),
                  (n, n + 1, 1, 1)]
    for _ in range(20):                                   # odd sizes, exact 8x and 1/8
        h, w = (int(v) * 2 + 1 for v in rng.integers(1, 40, 2))
        pairs += [(h, w, 8 * h, 8 * w - 1), (8 * h + 1, 8 * w, h, w)]
    for size, max_size in ((800, 1333), (600, 1000)):     # VG-like
        for _ in range(15):
            h, w = int(rng.integers(200, 1100)), int(rng.integers(200, 1100))
            pairs.append((h, w) + _target_size(h, w, size, max_size))
    return pairs


PAIRS = size_pairs()


def test_sweep_is_large_and_covers_the_cases():
    assert len(PAIRS) >= 200
    assert any(oh == 1 or ow == 1 for _, _, oh, ow in PAIRS) and any(h == 1 or w == 1 for h, w, _, _ in PAIRS)
    assert any(oh >= 8 * h for h, _, oh, _ in PAIRS) and any(8 * oh <= h for h, _, oh, _ in PAIRS)
    assert any(h == oh and w != ow for h, w, oh, ow in PAIRS)


@pytest.mark.parametrize("chunk", range(0, len(PAIRS), 25))
def test_restated_resize_equals_pillow_bit_for_bit(chunk):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(chunk)
    for h, w, oh, ow in PAIRS[chunk:chunk + 25]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        got = R.pil_resize(img, oh, ow)
        assert got.dtype == np.uint8 and got.shape == ref.shape
        assert np.array_equal(got, ref), (h, w, oh, ow)


def test_coefficients_are_pillows_integers():
    bounds, weights = pil_bilinear_coeffs(5, 3)
    assert bounds.dtype == np.int32 and weights.dtype == np.int32 and weights.shape == (3, 5)
    assert np.array_equal(bounds[:, 0], [0, 1, 3]) and np.array_equal(bounds[:, 1], [3, 3, 2])
    # every row's weights sum to 2^22 up to the per-weight rounding
    for n_in, n_out in ((5, 3), (3, 7), (1333, 800), (17, 1), (1, 9)):
        b, k = pil_bilinear_coeffs(n_in, n_out)
        assert (k >= 0).all() and (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] >= 1).all()
        assert (k[np.arange(k.shape[1])[None, :] >= b[:, 1:]] == 0).all()
    with pytest.raises(ValueError):
        pil_bilinear_coeffs(0, 4)


def test_lut_is_the_418_float32_formula_and_not_u_over_255():
    lut = normalize_lut()
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    u = np.arange(256, dtype=np.float32)
    mean = np.array(FE.IMAGENET_MEAN).astype(np.float32)[:, None]
    std = np.array(FE.IMAGENET_STD).astype(np.float32)[:, None]
    expect = ((u * np.float32(1 / 255.0))[None, :] - mean) / std
    assert np.array_equal(lut.view(np.int32), expect.view(np.int32))
    divided = ((u / np.float32(255.0))[None, :] - mean) / std
    assert (u * np.float32(1 / 255.0) != u / np.float32(255.0)).sum() == 126
    assert (lut != divided).sum() == 322
    # the restated normalise uses the same table
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 256, 3)
    assert np.array_equal(R.normalize(img)[:, 0, :], lut)


def test_golden_is_reproduced_by_the_restatement(golden_dir):
    g = np.load(os.path.join(golden_dir, "preprocess.npz"))
    shapes = [tuple(s) for s in g["shapes"]]
    flat, images, o = g["pixels"], [], 0
    for h, w in shapes:
        images.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    assert o == flat.size
    pv, pm = R.preprocess(images, int(g["size"]), int(g["max_size"]))
    assert pv.shape == g["pixel_values"].shape and pm.dtype == np.int64
    assert np.array_equal(pv.view(np.int32), g["pixel_values"].view(np.int32))
    assert np.array_equal(pm, g["pixel_mask"])
    # the golden has an identity axis, an upscale, a downscale, a 1-pixel row and a width that is not a multiple of 4
    outs = [_target_size(h, w, int(g["size"]), int(g["max_size"])) for h, w in shapes]
    assert any(o == s for o, s in zip(outs, shapes)) and pv.shape[-1] % 4 != 0
    assert any(h == 1 for h, _ in shapes)


def test_output_sizes_and_labels_match_the_existing_extractor():
    rng = np.random.default_rng(3)
    dev_fe, host_fe = DeformableDetrDeviceFeatureExtractor(), DeformableDetrFeatureExtractor()
    for h, w in ((375, 500), (500, 333), (1024, 768), (600, 800), (37, 2000)):
        n = 5
        xy = torch.from_numpy(rng.uniform(0, min(h, w) / 2, (n, 2)).astype(np.float32))
        boxes = torch.cat([xy, xy + torch.from_numpy(rng.uniform(1, min(h, w) / 2, (n, 2)).astype(np.float32))], 1)
        ann = {"boxes": boxes, "class_labels": torch.arange(n), "image_id": torch.tensor([h])}
        ref = host_fe(torch.zeros(3, h, w), annotations=ann)
        got = dev_fe.targets([(h, w)], [ann])[0]
        exp = ref["labels"][0]
        assert dev_fe.output_size(h, w) == _target_size(h, w, 800, 1333) == tuple(ref["pixel_values"].shape[-2:])
        assert sorted(got) == sorted(exp)
        for k in exp:
            assert torch.equal(got[k], exp[k]), k
    # do_resize=False keeps the size, like the host extractor
    fe = DeformableDetrDeviceFeatureExtractor(do_resize=False)
    assert fe.output_size(123, 45) == (123, 45)
    ann = {"boxes": torch.tensor([[1.0, 2.0, 30.0, 40.0]])}
    exp = DeformableDetrFeatureExtractor(do_resize=False)(torch.zeros(3, 123, 45), annotations=ann)["labels"][0]
    got = fe.targets([(123, 45)], [ann])[0]
    assert sorted(got) == sorted(exp) and all(torch.equal(got[k], exp[k]) for k in exp)


def test_do_normalize_false_and_bad_images_are_refused():
    with pytest.raises(NotImplementedError):
        DeformableDetrDeviceFeatureExtractor(do_normalize=False).prepare([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        FE._as_hwc_uint8(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        FE._as_hwc_uint8(torch.zeros(4, 4, 4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        FE._as_hwc_uint8([[1, 2, 3]])


def test_device_tables_and_routes():
    """The identity table reproduces a skipped pass; the widest tile window decides the fallback route."""
    flat, k, window = FE._device_table(7, 7)
    assert k == 1 and np.array_equal(flat[:14].reshape(7, 2), np.stack([np.arange(7), np.ones(7)], 1))
    assert (flat[14:] == 1 << 22).all() and window == 3 * 7
    _, _, window = FE._device_table(800, 1066)
    assert window <= FE.PREPROCESS_STAGE_BYTES
    _, _, window = FE._device_table(7200, 144)
    assert window > FE.PREPROCESS_STAGE_BYTES
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "egtr_hip.h")).read()
    assert int(re.search(r"EGTR_PREPROCESS_TILE_W (\d+)", hdr).group(1)) == FE.PREPROCESS_TILE_W
    assert int(re.search(r"EGTR_PREPROCESS_STAGE_BYTES (\d+)", hdr).group(1)) == FE.PREPROCESS_STAGE_BYTES
