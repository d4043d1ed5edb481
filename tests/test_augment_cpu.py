"""CPU: the reference's training augmentation as the device extractors run it, checked on the host -- the draws of
sample_augmentation and the target arithmetic of augment_target against the fixture recorded from the reference's own
chain (tests/golden/make_golden_augment.py), the numpy restatement of the kernels' pixel path
(tests/augment_restated.py) against Pillow's transpose / resize / crop / resize and against the fixture, and the C
entries' argument checks."""
import hashlib
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import augment_restated as A  # noqa: E402
import pil_resample_restated as R  # noqa: E402

from egtr_amd import feature_extraction as FE  # noqa: E402
from egtr_amd.feature_extraction import (AugmentParams, DeformableDetrDeviceFeatureExtractorWithAugmentor,  # noqa: E402
                                         DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop, augment_target,
                                         sample_augmentation)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def fixture_cases(g):
    """(prefix, constants, crop variant, (h, w), seed, case index under the prefix, input boxes) of every stored case."""
    small, full = A.fixture_constants(g, "small"), A.fixture_constants(g, "full")
    base = int(g["small_seed_base"])
    for prefix, crop in (("small_nocrop_", False), ("small_crop_", True)):
        for i, (h, w) in enumerate(g["small_shapes"]):
            yield prefix, small, crop, (int(h), int(w)), base + i, i, g["small_in_boxes"][i]
    base = int(g["full_seed_base"])
    for i, (h, w) in enumerate(g["full_shapes"]):
        yield "full_", full, bool(g["full_crop"][i]), (int(h), int(w)), base + i, i, g["full_in_boxes"][i]


def test_fixture_covers_the_cases(g):
    assert len(g["full_shapes"]) >= 200 and len(g["small_shapes"]) >= 12
    for prefix in ("small_nocrop_", "small_crop_", "full_"):
        assert {(int(r[0]), int(r[1])) for r in g[prefix + "params"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (g["small_nocrop_params"][:, 4] < 0).all()
    rows = np.concatenate([g["small_crop_params"], g["full_params"]])
    assert any(r[4] >= 0 and tuple(r[6:8]) == tuple(r[2:4]) for r in rows)            # a crop equal to the image
    shapes = np.concatenate([g["small_shapes"], g["full_shapes"]])
    assert any(r[1] == 1 and tuple(r[2:4]) == tuple(s) for r, s in zip(rows, shapes))  # an identity first resize
    assert (g["small_crop_n_out"] < g["small_in_boxes"].shape[1]).any()                # a crop that drops a box
    assert (g["full_n_out"] < g["full_in_boxes"].shape[1]).any()


def test_sampling_reproduces_the_reference_draws(g):
    """Same flips, branches, sizes and crop regions, and both generators left in the same state."""
    n = 0
    for prefix, consts, crop, (h, w), seed, i, _ in fixture_cases(g):
        random.seed(seed)
        torch.manual_seed(seed)
        got = sample_augmentation(h, w, crop, **consts)
        assert got == A.fixture_params(g[prefix + "params"][i], g[prefix + "size2"][i]), (prefix, i, got)
        nxt = (random.random(), float(torch.rand(1, dtype=torch.float64)))
        assert nxt == tuple(g[prefix + "next"][i]), (prefix, i)
        n += 1
    assert n >= 224


def test_extractor_samples_in_batch_order(g):
    consts = A.fixture_constants(g, "small")
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentor(max_size=consts["max_size"], scales=consts["scales"],
                                                           mid_sizes=consts["mid_sizes"], crop_range=consts["crop_range"])
    shapes = [(int(h), int(w)) for h, w in g["small_shapes"]]
    random.seed(5)
    torch.manual_seed(5)
    got = [fe.sample(h, w) for h, w in shapes]
    random.seed(5)
    torch.manual_seed(5)
    assert got == [sample_augmentation(h, w, True, **consts) for h, w in shapes]
    assert DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop.use_crop is False
    d = DeformableDetrDeviceFeatureExtractorWithAugmentor()
    assert (list(d.scales), d.mid_sizes, d.crop_range, d.max_size) == (list(range(480, 801, 32)), (400, 500, 600),
                                                                       (384, 600), 1333)


def test_targets_equal_the_reference(g):
    dropped = 0
    for prefix in ("small_nocrop_", "small_crop_"):
        for i, (exp, (h, w)) in enumerate(zip(A.output_targets(g, prefix), g["small_shapes"])):
            h, w, boxes = int(h), int(w), g["small_in_boxes"][i]
            p = A.fixture_params(g[prefix + "params"][i], g[prefix + "size2"][i])
            got = augment_target(A.input_target(boxes), h, w, p, normalize=False)
            for k in exp:
                assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), (prefix, i, k)
            assert torch.equal(got["orig_size"], torch.tensor([h, w]))
            dropped += len(boxes) - len(got["boxes"])
            # the default also applies the extractor's cxcywh normalisation by the final size
            norm = augment_target(A.input_target(boxes), h, w, p)
            ref = FE.DeformableDetrFeatureExtractor._normalize_target(dict(exp), *p.size2)
            assert torch.equal(norm["boxes"], ref["boxes"]) and tuple(norm["size"].tolist()) == p.size2
    assert dropped > 0


def test_targets_equal_the_reference_at_full_size(g):
    exp_all = A.output_targets(g, "full_")
    dropped = 0
    for i, (h, w) in enumerate(g["full_shapes"]):
        p = A.fixture_params(g["full_params"][i], g["full_size2"][i])
        got = augment_target(A.input_target(g["full_in_boxes"][i]), int(h), int(w), p, normalize=False)
        for k in exp_all[i]:
            assert got[k].dtype == exp_all[i][k].dtype and torch.equal(got[k], exp_all[i][k]), (i, k)
        dropped += 5 - len(got["boxes"])
    assert dropped > 0
    # optional fields stay optional
    p = AugmentParams(True, (40, 50), (3, 4, 20, 30), (30, 45))
    got = augment_target({"boxes": torch.tensor([[60.0, 10.0, 95.0, 40.0]]), "class_labels": torch.tensor([2])}, 80, 100, p)
    assert "iscrowd" not in got and got["boxes"].shape == (1, 4) and torch.equal(got["orig_size"], torch.tensor([80, 100]))
    assert augment_target(None, 80, 100, p) is None


# ---- pixels: the restatement against Pillow on enumerated parameter sets ---------------------------------------------
SCENARIOS = [  # (h, w), first resize (h1, w1), final-size factors (fh, fw)
    ((30, 40), (30, 40), (1.5, 1.5)),      # identity first resize, upscale
    ((30, 40), (30, 40), (1.0, 1.0)),      # nothing resampled at all
    ((48, 36), (32, 24), (2.0, 2.0)),      # down, then up
    ((25, 37), (50, 74), (0.5, 0.5)),      # up, then down
    ((40, 64), (40, 51), (1.3, 1.3)),      # identity vertical axis in the first resize
    ((64, 40), (51, 40), (0.7, 0.7)),      # identity horizontal axis in the first resize
    ((33, 47), (21, 30), (1.0, 1.7)),      # identity vertical axis in the final resize (crop-free sets)
    ((61, 29), (40, 19), (3.1, 2.9)),
    ((20, 90), (24, 108), (0.4, 0.45)),
    ((77, 53), (10, 7), (4.0, 4.0)),       # 8x down, 4x up
    ((9, 11), (70, 85), (0.2, 0.2)),       # 8x up, 5x down
    ((45, 45), (45, 60), (1.0, 1.0)),
    ((52, 38), (26, 19), (1.9, 2.3)),
    ((31, 64), (44, 91), (0.8, 0.6)),
]
CROPS = ["none", "inner", "left", "right", "top", "bottom", "full"]


def crop_region(kind, h1, w1):
    ch, cw = max(1, h1 // 2), max(1, w1 // 2)
    return {"none": None, "inner": (h1 // 4, w1 // 4, ch, cw), "left": (h1 // 4, 0, ch, cw),
            "right": (h1 // 4, w1 - cw, ch, cw), "top": (0, w1 // 4, ch, cw), "bottom": (h1 - ch, w1 // 4, ch, cw),
            "full": (0, 0, h1, w1)}[kind]


def enumerated_sets():
    """flip x (one resize | two resizes x every crop kind) x every scenario."""
    sets = []
    for (h, w), s1, (fh, fw) in SCENARIOS:
        for flip in (False, True):
            sets.append(((h, w), AugmentParams(flip, None, None, (max(1, int(h * fh)), max(1, int(w * fw))))))
            for kind in CROPS:
                region = crop_region(kind, *s1)
                wh, ww = region[2:] if region else s1
                sets.append(((h, w), AugmentParams(flip, s1, region, (max(1, int(wh * fh)), max(1, int(ww * fw))))))
    return sets


SETS = enumerated_sets()


def test_enumeration_is_complete():
    assert len(SETS) == len(SCENARIOS) * 2 * (1 + len(CROPS)) >= 200
    assert any(p.size1 == hw for hw, p in SETS) and any(p.size1 is None and p.size2 == hw for hw, p in SETS)
    assert any(p.size1 and p.size1[0] > 2 * hw[0] for hw, p in SETS) and any(p.size1 and 2 * p.size1[0] < hw[0] for hw, p in SETS)


@pytest.mark.parametrize("chunk", range(0, len(SETS), 32))
def test_restatement_equals_pillow_bit_for_bit(chunk):
    rng = np.random.default_rng(chunk)
    for (h, w), p in SETS[chunk:chunk + 32]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got, ref = A.augment_image(img, p), A.pillow_chain(img, p)
        assert got.dtype == np.uint8 and got.shape == ref.shape == p.size2 + (3,)
        assert np.array_equal(got, ref), ((h, w), p)


def test_pass_axis_is_resample_axis_on_a_whole_unmirrored_axis():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for out, axis in ((80, 1), (11, 1), (90, 0), (5, 0)):
        full = R.resample_axis(a, out, axis)
        assert np.array_equal(A.pass_axis(a, out, axis), full)
        lo, n = out // 3, out // 2
        assert np.array_equal(A.pass_axis(a, out, axis, lo, n), np.take(full, np.arange(lo, lo + n), axis))
        assert np.array_equal(A.pass_axis(a, out, axis, mirror=True), R.resample_axis(np.flip(a, axis), out, axis))


def test_restatement_equals_the_fixture_pixels(g):
    images = A.small_images(g)
    for prefix in ("small_nocrop_", "small_crop_"):
        params = [A.fixture_params(r, s) for r, s in zip(g[prefix + "params"], g[prefix + "size2"])]
        pv, pm = A.augment_batch(images, params)
        assert pv.shape == g[prefix + "pixel_values"].shape
        assert np.array_equal(pv.view(np.int32), g[prefix + "pixel_values"].view(np.int32))
        assert np.array_equal(pm, g[prefix + "pixel_mask"].astype(np.int64))


def test_restatement_equals_the_full_size_hashes(g):
    base = int(g["full_seed_base"])
    kinds = set()
    for i, sha in enumerate(g["full_sha256"]):
        h, w = (int(v) for v in g["full_shapes"][i])
        img = np.random.default_rng(base + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = A.fixture_params(g["full_params"][i], g["full_size2"][i])
        out = A.augment_image(img, p)
        assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == str(sha), (i, p)
        kinds.add((p.flip, p.size1 is not None))
    assert len(g["full_sha256"]) >= 4 and len(kinds) >= 2


def test_no_augmentation_parameters_are_the_evaluation_preprocessing():
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((75, 100), (100, 66), (40, 200))]
    params = [AugmentParams(False, None, None, FE._target_size(*img.shape[:2], 120, 200)) for img in images]
    pv, pm = A.augment_batch(images, params)
    ref_pv, ref_pm = R.preprocess(images, 120, 200)
    assert np.array_equal(pv.view(np.int32), ref_pv.view(np.int32)) and np.array_equal(pm, ref_pm)


def test_bad_parameters_are_refused():
    with pytest.raises(ValueError):
        AugmentParams(False, None, (0, 0, 4, 4), (8, 8))
    chk = DeformableDetrDeviceFeatureExtractorWithAugmentor._check
    with pytest.raises(ValueError):
        chk(AugmentParams(False, (10, 10), (5, 5, 6, 5), (8, 8)))
    with pytest.raises(ValueError):
        chk(AugmentParams(False, None, None, (0, 8)))
    chk(AugmentParams(True, (10, 10), (5, 5, 5, 5), (8, 8)))


def test_window_bytes_decide_the_prepass_route():
    b, _ = FE.pil_bilinear_coeffs(7200, 144)
    assert FE._window_bytes(b, 0, 144) > FE.PREPROCESS_STAGE_BYTES
    assert FE._window_bytes(b, 10, 20) < FE._window_bytes(b, 0, 144)
    b, _ = FE.pil_bilinear_coeffs(500, 1066)
    assert FE._window_bytes(b, 0, 1066) == FE._device_table(500, 1066)[2] <= FE.PREPROCESS_STAGE_BYTES
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "egtr_hip.h")).read()
    assert int(re.search(r"EGTR_AUGMENT_DESC_WORDS (\d+)", hdr).group(1)) == FE._AUG_DESC_WORDS
    for name, v in (("MIRROR", FE._AUG_MIRROR), ("SRC_WORKSPACE", FE._AUG_SRC_WS), ("PREPASS", FE._AUG_PREPASS)):
        assert int(re.search(r"EGTR_AUGMENT_%s (\d+)" % name, hdr).group(1)) == v


def test_coefficient_cache_appends_only_new_tables_and_stays_bounded(monkeypatch):
    """A lookup builds and copies the new tables only (no host copy of what is cached), tables keep their offsets when
    the buffer grows, and at MAX_INTS the cache starts afresh: a stream of random training sizes costs O(new tables)
    per batch and bounded memory."""
    built = []
    real = FE._device_table
    monkeypatch.setattr(FE, "_device_table", lambda a, b: built.append((a, b)) or real(a, b))
    monkeypatch.setattr(FE._CoeffCache, "MAX_INTS", 40000)
    monkeypatch.setattr(FE._CoeffCache, "MIN_INTS", 1024)
    cache = FE._CoeffCache("cpu")
    assert not hasattr(cache, "host")
    rng = np.random.default_rng(0)
    resets, seen = 0, {}
    for step in range(300):
        pairs = [(int(a), int(b)) for a, b in rng.integers(20, 90, (6, 2))] + [(64, 48)]
        before, used = len(built), cache.used
        known = [p for p in dict.fromkeys(pairs) if p in cache.index]
        buf, tabs = cache.lookup(pairs)
        if cache.used < used:                                   # started afresh: this batch's tables only
            resets += 1
            assert len(built) - before <= 2 * len(set(pairs)) and cache.used <= sum(len(real(*p)[0]) for p in set(pairs))
        else:
            assert len(built) - before == len(set(pairs)) - len(known)
        assert buf.numel() <= 40000 and cache.used <= buf.numel()
        for p, (off, k, window) in zip(pairs, tabs):
            flat, rk, rwindow = real(*p)
            assert (k, window) == (rk, rwindow) and np.array_equal(buf[off:off + len(flat)].numpy(), flat)
            assert np.array_equal(cache.bounds[p], flat[:2 * p[1]].reshape(-1, 2))
    assert resets >= 2


def test_null_arguments_are_rejected_without_a_gpu():
    """Argument validation happens before any HIP call, so it is checkable on a CPU-only box."""
    from egtr_amd import _lib
    h = _lib.lib()
    assert h.egtr_abi_version() == 7
    for entry in (h.egtr_preprocess_augment_f32, h.egtr_preprocess_augment_bf16):
        assert entry(None, None, None, 1, None, None, 8, 8, 0, 0, 0, 0, 0, 0, None, None, None) == -1
        # a first pass without its descriptors or its workspace, on otherwise non-null (never dereferenced) arguments
        assert entry(None, None, 16, 1, 16, 16, 8, 8, 4, 4, 0, 0, 0, 0, 16, 16, 16) == -1
        assert entry(None, 16, 16, 1, 16, 16, 8, 8, 4, 4, 0, 0, 0, 0, None, 16, 16) == -1
        assert entry(None, 16, 16, 0, 16, 16, 8, 8, 0, 0, 0, 0, 0, 0, None, 16, 16) == -1
        assert entry(None, 16, 16, 1, 16, 16, 8, 8, 4, 0, 0, 0, 0, 0, 16, 16, 16) == -1
