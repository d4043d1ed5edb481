"""GPU: DeformableDetrDeviceFeatureExtractor (csrc/preprocess.hip) -- bit-exact against the committed golden of the
reference's preprocessing and against the numpy restatement + the existing host pad on mixed VG-sized batches and on
extreme ratios that take the workspace route; bf16 output, device-resident input and graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pil_resample_restated as R  # noqa: E402

from egtr_amd.feature_extraction import (DeformableDetrDeviceFeatureExtractor,  # noqa: E402
                                         DeformableDetrFeatureExtractor)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def seeded_images(shapes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in shapes:
        # smooth gradients plus noise: realistic neighbourhoods, every byte value, clipping on both ends
        yy, xx = np.meshgrid(np.linspace(-40, 300, h), np.linspace(-40, 300, w), indexing="ij")
        base = np.stack([yy, xx, (yy + xx) / 2], -1) + rng.normal(0, 30, (h, w, 3))
        out.append(np.clip(base, 0, 255).astype(np.uint8))
    return out


def host_reference(images, size, max_size):
    """The restated per-image resize + normalise, batched by the existing extractor's host pad."""
    outs = []
    for img in images:
        oh, ow = DeformableDetrDeviceFeatureExtractor(size=size, max_size=max_size).output_size(*img.shape[:2])
        outs.append(torch.from_numpy(R.normalize(R.pil_resize(img, oh, ow))))
    return DeformableDetrFeatureExtractor().pad_and_create_pixel_mask(outs)


def assert_bit_equal(enc, ref):
    pv, pm = enc["pixel_values"], enc["pixel_mask"]
    assert pv.device.type == "cuda" and pm.dtype == torch.int64
    assert pv.shape == ref["pixel_values"].shape and pm.shape == ref["pixel_mask"].shape
    assert torch.equal(pv.cpu().view(torch.int32), ref["pixel_values"].view(torch.int32))
    assert torch.equal(pm.cpu(), ref["pixel_mask"])


def test_golden_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "preprocess.npz"))
    images, o = [], 0
    for h, w in g["shapes"]:
        images.append(g["pixels"][o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    fe = DeformableDetrDeviceFeatureExtractor(size=int(g["size"]), max_size=int(g["max_size"]))
    enc = fe(images, device=DEV)
    assert_bit_equal(enc, {"pixel_values": torch.from_numpy(g["pixel_values"]),
                           "pixel_mask": torch.from_numpy(g["pixel_mask"])})


@pytest.mark.parametrize("size,max_size", [(800, 1333), (600, 1000)])
def test_vg_sized_batches_equal_the_restatement(size, max_size):
    shapes = [(375, 500), (500, 333), (768, 1024), (600, 800), (1024, 683), (333, 500)]
    images = seeded_images(shapes, seed=size)
    enc = DeformableDetrDeviceFeatureExtractor(size=size, max_size=max_size)(images, device=DEV)
    assert_bit_equal(enc, host_reference(images, size, max_size))


def test_extreme_ratios_take_the_workspace_route_and_stay_exact():
    shapes = [(1500, 7200), (4000, 20), (2, 3), (45, 2500), (1, 1)]
    images = seeded_images(shapes, seed=11)
    fe = DeformableDetrDeviceFeatureExtractor(size=30, max_size=150)
    batch = fe.prepare(images, DEV)
    routes = batch.desc.cpu()[:, 10].tolist()
    assert routes[0] == 1 and routes[2] == 0 and batch.workspace is not None
    assert_bit_equal(batch.run(), host_reference(images, 30, 150))


def test_bf16_is_the_rounded_fp32_output():
    images = seeded_images([(375, 500), (480, 640), (97, 131)], seed=5)
    fe = DeformableDetrDeviceFeatureExtractor()
    f32 = fe(images, device=DEV)
    bf = fe(images, device=DEV, dtype=torch.bfloat16)
    assert bf["pixel_values"].dtype == torch.bfloat16
    assert torch.equal(bf["pixel_values"].view(torch.int16), f32["pixel_values"].to(torch.bfloat16).view(torch.int16))
    assert torch.equal(bf["pixel_mask"], f32["pixel_mask"])


def test_device_resident_input_equals_host_input():
    images = seeded_images([(375, 500), (600, 800), (61, 47)], seed=9)
    fe = DeformableDetrDeviceFeatureExtractor()
    host = fe(images, device=DEV)
    big = torch.from_numpy(seeded_images([(700, 900)], seed=1)[0]).to(DEV)
    on_dev = [torch.from_numpy(x).to(DEV) for x in images]
    big[:61, 3:50] = on_dev[2]
    on_dev[2] = big[:61, 3:50]                     # a strided view (row stride 900 * 3), read in place
    assert on_dev[2].stride() == (2700, 3, 1)
    dev = fe(on_dev)
    assert torch.equal(dev["pixel_values"].view(torch.int32), host["pixel_values"].view(torch.int32))
    assert torch.equal(dev["pixel_mask"], host["pixel_mask"])
    # torch host tensors and PIL-free numpy give the same as well
    tens = fe([torch.from_numpy(x) for x in images], device=DEV)
    assert torch.equal(tens["pixel_values"], host["pixel_values"])


def test_graph_capture_replay_equals_eager():
    images = seeded_images([(75, 100), (50, 33), (1500, 7200)], seed=13)
    fe = DeformableDetrDeviceFeatureExtractor(size=30, max_size=150)
    batch = fe.prepare(images, DEV)
    assert batch.workspace is not None        # the prepass launch is captured too
    eager = batch.run()
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
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pv.view(torch.int32), eager["pixel_values"].view(torch.int32))
    assert torch.equal(pm, eager["pixel_mask"])


def test_labels_and_single_image():
    img = seeded_images([(300, 400)], seed=2)[0]
    ann = {"boxes": torch.tensor([[10.0, 20.0, 110.0, 220.0]]), "class_labels": torch.tensor([3])}
    fe = DeformableDetrDeviceFeatureExtractor()
    enc = fe(img, annotations=ann, device=DEV)
    assert enc["pixel_values"].shape == (1, 3, 800, 1066)
    ref = DeformableDetrFeatureExtractor()(torch.zeros(3, 300, 400), annotations=ann)["labels"][0]
    assert all(torch.equal(enc["labels"][0][k], ref[k]) for k in ref)
