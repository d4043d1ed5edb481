"""Training-augmentation timing on one GPU (DeformableDetrDeviceFeatureExtractorWithAugmentor, csrc/augment.hip).
Prints one JSON line.  Inputs are VG-like uint8 images (375 x 500, 500 x 375, 333 x 500, 768 x 1024 in rotation); per
batch size (4 and 8) and per parameter set
  one_resize   every image on the one-resize branch, half of them flipped
  two_resize   every image on the two-resize branch with a crop, half of them flipped
  sampled      parameters drawn by sample_augmentation under a seed (the mix a training loader sees)
it reports
  launch_us            stream time of one prepared batch (device events around back-to-back AugmentBatch.run calls)
  plain_launch_us      the same for egtr_preprocess_f32 producing outputs of the same sizes from the same raw images:
                       the non-augmented cost of the evaluation-time kernel
  call_images_s        whole calls from uint8 numpy images (sampling, pinned packing, one H2D copy, the launches) over
                       a few dozen calls on a fresh coefficient cache: a short-run figure, see sampled_long_*
  bytes / roofline_us  algorithmic bytes (uint8 in, fp32 out, int64 mask, plus one uint8 write and read of the window on
                       the two-resize branch) / HBM_PEAK_GBS
and once
  sampled_long_crop / sampled_long_nocrop   --long-batches sampled bs-4 calls on distinct batches (long_sampled_run): ms
                       per call per window of 250, images/s of the first, last and worst window, and the coefficient
                       cache's buffer size, table count and resets.  This is the rate a training run sees.
  host_images_s_1cpu / host_images_s_pool   the reference's chain in Pillow + the 4.18 float32 normalise in numpy on the
                       sampled parameters, in this process and over --procs worker processes
  train_step_images_s  the images/s of profiles/r06_bench.json's train_step, and the worst long-run window over it

    python tools/augment_bench.py [--iters 50] [--procs 16] [--long-batches 4000]"""
import argparse
import json
import multiprocessing
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
SHAPES = [(375, 500), (500, 375), (333, 500), (768, 1024)]
MEAN = np.array((0.485, 0.456, 0.406)).astype(np.float32)[:, None, None]
STD = np.array((0.229, 0.224, 0.225)).astype(np.float32)[:, None, None]


def images(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, SHAPES[i % len(SHAPES)] + (3,), dtype=np.uint8) for i in range(n)]


def parameter_sets(imgs):
    from egtr_amd.feature_extraction import AugmentParams, _target_size, sample_augmentation
    one, two = [], []
    for i, a in enumerate(imgs):
        h, w = a.shape[:2]
        scale = (480, 800, 640, 736)[i % 4]
        one.append(AugmentParams(i % 2, None, None, _target_size(h, w, scale, 1333)))
        s1 = _target_size(h, w, (400, 500, 600)[i % 3], None)
        ch, cw = min(s1[0], 384 + 40 * (i % 5)), min(s1[1], 600 - 30 * (i % 5))
        region = ((s1[0] - ch) // 2, (s1[1] - cw) // 2, ch, cw)
        two.append(AugmentParams(i % 2, s1, region, _target_size(ch, cw, scale, 1333)))
    random.seed(1)
    torch.manual_seed(1)
    sampled = [sample_augmentation(a.shape[0], a.shape[1], True) for a in imgs]
    return {"one_resize": one, "two_resize": two, "sampled": sampled}


def host_chain(job):
    """The reference's per-image path for one (image, parameters): Pillow transpose / resize / crop / resize, then the
    4.18 float32 rescale and normalise."""
    from PIL import Image
    a, (flip, size1, crop, size2) = job
    im = Image.fromarray(a)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if size1 is not None:
        im = im.resize(size1[::-1], Image.BILINEAR)
        if crop is not None:
            im = im.crop((crop[1], crop[0], crop[1] + crop[3], crop[0] + crop[2]))
    v = np.array(im.resize(size2[::-1], Image.BILINEAR)).astype(np.float32) * (1 / 255.0)
    return ((v.transpose(2, 0, 1) - MEAN) / STD).shape


def host_rates(imgs, params, procs, rounds=4):
    jobs = [(a, (p.flip, p.size1, p.crop, p.size2)) for a, p in zip(imgs, params)] * rounds
    t0 = time.perf_counter()
    for j in jobs:
        host_chain(j)
    single = len(jobs) / (time.perf_counter() - t0)
    with multiprocessing.get_context("spawn").Pool(procs) as pool:
        pool.map(host_chain, jobs[:procs])                      # start the workers and import PIL outside the timing
        t0 = time.perf_counter()
        pool.map(host_chain, jobs * 4, chunksize=1)
        pooled = 4 * len(jobs) / (time.perf_counter() - t0)
    return single, pooled


def long_sampled_run(fe, dev, batches, bs=4, window=250, seed=3):
    """Sampled calls over thousands of distinct batches, the state training is in after its first minutes: images are
    drawn from 160 (70 % the four VG shapes, 30 % random 200..1100 shapes), every call samples its own parameters, so
    nearly every call brings new (in, out) size pairs to the coefficient cache.  Host clock around windows of calls that
    end in a synchronise; reports ms per call per window, and the cache's size."""
    from egtr_amd import feature_extraction as FE
    rng = np.random.default_rng(seed)
    shapes = [SHAPES[i % len(SHAPES)] if rng.random() < 0.7 else tuple(int(v) for v in rng.integers(200, 1100, 2))
              for i in range(160)]
    pool = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    random.seed(seed)
    torch.manual_seed(seed)
    cache = FE._COEFF_CACHES.setdefault(dev, FE._CoeffCache(dev))
    per_window, resets, used, tables = [], 0, cache.used, 0
    for start in range(0, batches, window):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(min(window, batches - start)):
            fe([pool[i] for i in rng.integers(0, len(pool), bs)], device=dev)
            resets += cache.used < used
            used = cache.used
        torch.cuda.synchronize()
        per_window.append((time.perf_counter() - t0) * 1e3 / min(window, batches - start))
        tables = max(tables, len(cache.index))
    last = per_window[-1]
    return {"batches": batches, "bs": bs, "window": window, "ms_per_call_by_window": [round(v, 3) for v in per_window],
            "first_window_images_s": round(bs * 1e3 / per_window[0], 1), "last_window_images_s": round(bs * 1e3 / last, 1),
            "worst_window_images_s": round(bs * 1e3 / max(per_window), 1), "cache_resets": int(resets),
            "cache_buffer_mb": round(cache.buf.numel() * 4 / 2 ** 20, 1), "cache_tables_max": tables}


def event_time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--long-batches", type=int, default=4000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU")
    from egtr_amd.feature_extraction import (DeformableDetrDeviceFeatureExtractor,
                                             DeformableDetrDeviceFeatureExtractorWithAugmentor)
    dev = torch.device("cuda:0")
    fe = DeformableDetrDeviceFeatureExtractorWithAugmentor()

    class FixedSizes(DeformableDetrDeviceFeatureExtractor):
        """The evaluation-time extractor, told the output size of every image."""
        def prepare_sizes(self, imgs, sizes):
            it = iter(sizes)
            self.output_size = lambda h, w: next(it)
            return self.prepare(imgs, dev)

    pool = images(16, seed=1)
    res = {"tool": "augment_bench", "hbm_peak_gbs": HBM_PEAK_GBS, "input_shapes": SHAPES}
    for bs in (4, 8):
        imgs = pool[:bs]
        for name, params in parameter_sets(imgs).items():
            batch = fe.prepare(imgs, dev, params)
            enc = batch.run()
            pv, pm = enc["pixel_values"], enc["pixel_mask"]
            plain = FixedSizes().prepare_sizes(imgs, [p.size2 for p in params])
            assert (plain.H, plain.W) == (batch.H, batch.W)
            # alternate the two so that both see the same machine state
            launch, plain_launch = [], []
            for _ in range(3):
                launch.append(event_time(lambda: batch.run(pv, pm), args.iters * 4))
                plain_launch.append(event_time(lambda: plain.run(pv, pm), args.iters * 4))
            subs = [pool[s * bs:(s + 1) * bs] for s in range(len(pool) // bs)]
            given = [None if name == "sampled" else parameter_sets(sub)[name] for sub in subs]
            k = [0]

            def call():
                k[0] = (k[0] + 1) % len(subs)
                fe(subs[k[0]], params=given[k[0]], device=dev)      # params=None: sampled inside the call
            us = event_time(call, args.iters)
            window = sum(2 * p.window()[2] * p.window()[3] * 3 for p in params if p.size1 is not None)
            nbytes = sum(a.size for a in imgs) + window + pv.numel() * 4 + pm.numel() * 8
            roof = nbytes / (HBM_PEAK_GBS * 1e9) * 1e6
            res[f"{name}_bs{bs}"] = {
                "launch_us": round(min(launch), 2), "launch_us_runs": [round(v, 2) for v in launch],
                "plain_launch_us": round(min(plain_launch), 2), "plain_launch_us_runs": [round(v, 2) for v in plain_launch],
                "launches": 1 + sum(1 for i in (0, 2, 4) if batch.extents[i]),
                "call_images_s": round(bs * 1e6 / us, 1), "bytes": int(nbytes), "roofline_us": round(roof, 2),
                "roofline_fraction": round(roof / min(launch), 3), "canvas": [batch.H, batch.W]}
    from egtr_amd.feature_extraction import DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop
    res["sampled_long_crop"] = long_sampled_run(fe, dev, args.long_batches)
    res["sampled_long_nocrop"] = long_sampled_run(DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop(), dev,
                                                  args.long_batches)
    sampled = parameter_sets(pool)["sampled"]
    single, pooled = host_rates(pool, sampled, args.procs)
    res["host_images_s_1cpu"], res["host_images_s_pool"], res["host_procs"] = round(single, 1), round(pooled, 1), args.procs
    try:
        ts = json.load(open(os.path.join(ROOT, "profiles", "r06_bench.json")))["train_step"]
        rate = float(ts["value"])                                  # images/s of the bs-4 train step
        res["train_step_images_s"] = round(rate, 1)
        res["sampled_long_worst_window_over_train_step"] = round(
            min(res[k]["worst_window_images_s"] for k in ("sampled_long_crop", "sampled_long_nocrop")) / rate, 1)
        res["host_pool_over_train_step"] = round(pooled / rate, 2)
    except (OSError, KeyError, TypeError) as e:
        res["train_step_images_s"] = f"not available ({type(e).__name__})"
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
