"""GPU: DeformableDetrDeviceFeatureExtractorWithAugmentor / ...NoCrop (csrc/augment.hip) -- bit-exact against the
fixture recorded from the reference's chain and against the numpy restatement of the kernels' pixel path
(tests/augment_restated.py) on VG-sized batches that mix every flip x branch, with sampled parameters, on the prepass
route, in bf16, from device-resident input and through graph capture."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import augment_restated as A  # noqa: E402
from augment_restated import seeded_images  # noqa: E402

from egtr_amd import feature_extraction as FE  # noqa: E402
from egtr_amd.feature_extraction import (AugmentParams, DeformableDetrDeviceFeatureExtractor,  # noqa: E402
                                         DeformableDetrDeviceFeatureExtractorWithAugmentor,
                                         DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop, _target_size,
                                         augment_target, sample_augmentation)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VG_SHAPES = [(375, 500), (500, 333), (768, 1024), (600, 800), (1024, 683), (333, 500)]


def assert_bit_equal(enc, pv, pm):
    got_pv, got_pm = enc["pixel_values"], enc["pixel_mask"]
    assert got_pv.device.type == "cuda" and got_pm.dtype == torch.int64
    assert tuple(got_pv.shape) == pv.shape and tuple(got_pm.shape) == pm.shape
    assert torch.equal(got_pv.cpu().view(torch.int32), torch.from_numpy(pv).view(torch.int32))
    assert torch.equal(got_pm.cpu(), torch.from_numpy(pm))


@pytest.mark.parametrize("prefix,cls", [("small_nocrop_", DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop),
                                        ("small_crop_", DeformableDetrDeviceFeatureExtractorWithAugmentor)])
def test_golden_bit_exact(golden_dir, prefix, cls):
    """The reference's chain under the fixture's seeds: sampled on the host, executed on the device."""
    g = np.load(os.path.join(golden_dir, "augment.npz"))
    c = A.fixture_constants(g, "small")
    fe = cls(max_size=c["max_size"], scales=c["scales"], mid_sizes=c["mid_sizes"], crop_range=c["crop_range"])
    images = A.small_images(g)
    params = []
    for i, img in enumerate(images):
        random.seed(int(g["small_seed_base"]) + i)
        torch.manual_seed(int(g["small_seed_base"]) + i)
        params.append(fe.sample(*img.shape[:2]))
    anns = [A.input_target(b) for b in g["small_in_boxes"]]
    enc = fe(images, annotations=anns, params=params, device=DEV)
    assert_bit_equal(enc, g[prefix + "pixel_values"], g[prefix + "pixel_mask"].astype(np.int64))
    for got, exp, p in zip(enc["labels"], A.output_targets(g, prefix), params):
        ref = FE.DeformableDetrFeatureExtractor._normalize_target(dict(exp), *p.size2)
        for k in ref:
            assert torch.equal(got[k], ref[k]), k


def mixed_params(shapes, crop):
    """All four flip x branch combinations inside one batch (and again with the roles shifted)."""
    params = []
    for i, (h, w) in enumerate(shapes):
        flip, two = bool(i & 1), bool(i & 2) != bool(i & 4)
        scale = (480, 800, 640, 704, 544, 768)[i % 6]
        if not two:
            params.append(AugmentParams(flip, None, None, _target_size(h, w, scale, 1333)))
            continue
        s1 = _target_size(h, w, (400, 500, 600)[i % 3], None)
        region = None
        if crop:
            ch, cw = min(s1[0], 384 + 31 * i), min(s1[1], 600 - 17 * i)
            region = ((s1[0] - ch) // 2 + (s1[0] - ch) % 2, s1[1] - cw if i & 1 else 0, ch, cw)
        wh, ww = region[2:] if region else s1
        params.append(AugmentParams(flip, s1, region, _target_size(wh, ww, scale, 1333)))
    return params


@pytest.mark.parametrize("crop", [False, True])
def test_vg_sized_mixed_batches_equal_the_restatement(crop):
    shapes = VG_SHAPES + [(600, 800), (480, 640)]       # (600, 800) at 600: an identity first resize
    images = seeded_images(shapes, seed=800 + crop)
    params = mixed_params(shapes, crop)
    params[6] = AugmentParams(True, (600, 800), (100, 150, 450, 600) if crop else None, params[6].size2)
    assert {(p.flip, p.size1 is not None) for p in params} == {(False, False), (True, False), (False, True), (True, True)}
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentor()
    batch = fe.prepare(images, DEV, params)
    assert batch.workspace is not None and batch.extents[0] > 0 and batch.extents[2:] == (0, 0, 0, 0)
    assert_bit_equal(batch.run(), *A.augment_batch(images, params))


@pytest.mark.parametrize("cls", [DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop,
                                 DeformableDetrDeviceFeatureExtractorWithAugmentor])
def test_sampled_parameters_under_a_seed(cls):
    images = seeded_images(VG_SHAPES, seed=21)
    boxes = [np.array([[10.0, 20.0, 110.0, 220.0], [0.0, 0.0, 30.0, 25.0], [w - 40.0, h - 30.0, w, h]], np.float32)
             for h, w in VG_SHAPES]
    anns = [A.input_target(b) for b in boxes]
    fe = cls()
    random.seed(77)
    torch.manual_seed(77)
    enc = fe(images, annotations=anns, device=DEV)
    random.seed(77)
    torch.manual_seed(77)
    params = [sample_augmentation(h, w, cls.use_crop) for h, w in VG_SHAPES]
    assert_bit_equal(enc, *A.augment_batch(images, params))
    for got, ann, (h, w), p in zip(enc["labels"], anns, VG_SHAPES, params):
        exp = augment_target(ann, h, w, p)
        assert sorted(got) == sorted(exp) and all(torch.equal(got[k], exp[k]) for k in exp)


def test_no_augmentation_equals_the_evaluation_extractor():
    images = seeded_images(VG_SHAPES, seed=3)
    ref = DeformableDetrDeviceFeatureExtractor()(images, device=DEV)
    params = [AugmentParams(False, None, None, _target_size(h, w, 800, 1333)) for h, w in VG_SHAPES]
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop()
    batch = fe.prepare(images, DEV, params)
    assert batch.workspace is None and batch.first is None and batch.extents == (0,) * 6
    enc = batch.run()
    assert torch.equal(enc["pixel_values"].view(torch.int32), ref["pixel_values"].view(torch.int32))
    assert torch.equal(enc["pixel_mask"], ref["pixel_mask"])


def test_extreme_ratio_takes_the_prepass_route_flipped_and_twice_resized():
    shapes = [(1500, 7200), (20, 7000), (64, 48), (4000, 20)]
    images = seeded_images(shapes, seed=11)
    params = [AugmentParams(True, (30, 144), (5, 10, 20, 130), (40, 200)),      # prepass in the first pass, mirrored
              AugmentParams(True, None, None, (3, 100)),                        # prepass in the only pass, mirrored
              AugmentParams(True, (32, 24), None, (40, 30)),
              AugmentParams(False, (4000, 20), None, (150, 1))]
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentor()
    batch = fe.prepare(images, DEV, params)
    flags = lambda d: [int(v) for v in d.cpu()[:, 14]]       # noqa: E731
    assert flags(batch.first)[0] == FE._AUG_MIRROR | FE._AUG_PREPASS and flags(batch.first)[2] == FE._AUG_MIRROR
    assert flags(batch.final)[1] == FE._AUG_MIRROR | FE._AUG_PREPASS and flags(batch.final)[0] == FE._AUG_SRC_WS
    by, _ = FE.pil_bilinear_coeffs(1500, 30)                  # the prepass covers the rows the crop window reads only
    rows = int(by[24, 0] + by[24, 1] - by[5, 0])
    assert rows < 1500 and batch.extents == (4000, 130, rows, 130, 20, 100)
    assert_bit_equal(batch.run(), *A.augment_batch(images, params))


def test_bf16_is_the_rounded_fp32_output():
    images = seeded_images(VG_SHAPES[:4], seed=5)
    params = mixed_params(VG_SHAPES[:4], True)
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentor()
    f32 = fe(images, params=params, device=DEV)
    bf = fe(images, params=params, device=DEV, dtype=torch.bfloat16)
    assert bf["pixel_values"].dtype == torch.bfloat16
    assert torch.equal(bf["pixel_values"].view(torch.int16), f32["pixel_values"].to(torch.bfloat16).view(torch.int16))
    assert torch.equal(bf["pixel_mask"], f32["pixel_mask"])


def test_device_resident_strided_input_equals_host_input():
    shapes = [(375, 500), (600, 800), (61, 47), (333, 500)]
    images = seeded_images(shapes, seed=9)
    params = mixed_params(shapes, False)
    params[2] = AugmentParams(True, (80, 61), (7, 9, 50, 40), (75, 60))
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentor()
    host = fe(images, params=params, device=DEV)
    big = torch.from_numpy(seeded_images([(700, 900)], seed=1)[0]).to(DEV)
    on_dev = [torch.from_numpy(x).to(DEV) for x in images]
    big[:61, 3:50] = on_dev[2]
    on_dev[2] = big[:61, 3:50]                     # a strided view (row stride 900 * 3), read in place, mirrored
    assert on_dev[2].stride() == (2700, 3, 1)
    dev = fe(on_dev, params=params)
    assert torch.equal(dev["pixel_values"].view(torch.int32), host["pixel_values"].view(torch.int32))
    assert torch.equal(dev["pixel_mask"], host["pixel_mask"])
    assert_bit_equal(host, *A.augment_batch(images, params))


def test_graph_capture_replay_equals_eager():
    shapes = [(375, 500), (500, 333), (20, 7000)]
    images = seeded_images(shapes, seed=13)
    params = [AugmentParams(True, (400, 533), (8, 100, 390, 420), (520, 560)),
              AugmentParams(False, None, None, (720, 480)), AugmentParams(True, None, None, (3, 100))]
    batch = DeformableDetrDeviceFeatureExtractorWithAugmentor().prepare(images, DEV, params)
    assert batch.workspace is not None and batch.extents[0] > 0 and batch.extents[4] > 0    # every launch kind but one
    eager = batch.run()
    assert_bit_equal(eager, *A.augment_batch(images, params))
    pv = torch.empty_like(eager["pixel_values"])
    pm = torch.empty_like(eager["pixel_mask"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.run(pv, pm)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch.run(pv, pm)
    pv.fill_(7.0)
    pm.fill_(7)
    batch.workspace.fill_(9)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pv.view(torch.int32), eager["pixel_values"].view(torch.int32))
    assert torch.equal(pm, eager["pixel_mask"])


def test_coefficient_cache_on_the_device_keeps_offsets_across_growth():
    cache = FE._CoeffCache(DEV)
    rng = np.random.default_rng(2)
    kept = []
    for step in range(40):
        pairs = [(int(a), int(b)) for a, b in rng.integers(100, 900, (5, 2))]
        buf, tabs = cache.lookup(pairs)
        kept += list(zip(pairs, tabs))
    assert cache.buf.numel() > FE._CoeffCache.MIN_INTS        # it grew, device to device
    host = cache.buf.cpu().numpy()
    for p, (off, k, window) in kept:
        flat, rk, rwindow = FE._device_table(*p)
        assert (k, window) == (rk, rwindow) and np.array_equal(host[off:off + len(flat)], flat)
