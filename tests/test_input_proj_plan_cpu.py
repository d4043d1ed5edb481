"""CPU: the plan of the grouped input-projection launch (egtr_input_proj_x6_workspace_floats, egtr_amd/csrc/input_proj_x6.hip) --
how many K ranges S_l each level is cut into -- over every image shape of bench.mixed_shape_set() at batch 1 and 600 x 1000 at
batch 8.  A function of the shapes alone: no device is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (512, 1024, 2048)      # ResNet-50 stages 2-4; the extra level is a 3x3 / stride 2 convolution of the last one


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(os.path.join(ROOT, "egtr_amd", "libegtr_hip.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "egtr_amd", "csrc"), "-j", "4"], check=True)
    from egtr_amd import ops
    return ops


def _half(n):
    return (n - 1) // 2 + 1


def _levels(B, H, W):
    """(rows, K, tap channels) of the four levels for a batch of B images of H x W"""
    h, w = _half(_half(H)), _half(_half(W))          # stem convolution + max-pool
    rows, K, tapc = [], [], []
    for c in CHANNELS:
        h, w = _half(h), _half(w)
        rows.append(B * h * w)
        K.append(c)
        tapc.append(0)
    rows.append(B * _half(h) * _half(w))
    K.append(9 * CHANNELS[-1])
    tapc.append(CHANNELS[-1])
    return rows, K, tapc


def _cases():
    import bench
    return [(1, h, w) for h, w in bench.mixed_shape_set()] + [(8, 600, 1000)]


def test_bench_shapes_are_what_the_plan_is_documented_for():
    assert _levels(1, 600, 1000)[0] == [75 * 125, 38 * 63, 19 * 32, 10 * 16]


def test_plan_partitions_k_within_the_limits_for_every_bench_shape(ops):
    for B, H, W in _cases():
        rows, K, tapc = _levels(B, H, W)
        splits, floats = ops.input_proj_x6_plan(rows, K, tapc)
        assert (splits, floats) == ops.input_proj_x6_plan(rows, K, tapc), "the same arguments give the same plan"
        assert floats == sum(s * r * 256 for s, r in zip(splits, rows))
        for s, k, c in zip(splits, K, tapc):
            assert s >= 1 and k % s == 0, "equal pieces that partition K exactly"
            piece = k // s
            assert piece % 32 == 0 and piece <= 512
            assert c == 0 or c % piece == 0, "no piece straddles a tap"
            # the split form's error bound (6 K_s / 16 + 4 + S) 2^-23 is not larger than the unsplit (6 K / 16 + 4) 2^-23
            assert s == 1 or 16 * s <= 6 * (k - piece)
        units = sum(2 * ((r + 63) // 64) * s for r, s in zip(rows, splits))
        base = sum(2 * ((r + 63) // 64) * -(-k // 512) for r, k in zip(rows, K))
        assert units == base or units <= 1024, "splitting beyond the K limit stays within two resident rounds"


def test_plan_at_the_bench_shape(ops):
    """the unit counts written next to the rule in input_proj_x6.hip"""
    assert ops.input_proj_x6_plan(*_levels(1, 600, 1000))[0] == [1, 4, 8, 36]
    assert ops.input_proj_x6_plan(*_levels(8, 600, 1000))[0] == [1, 2, 4, 36]


def test_unserved_shapes_have_no_plan(ops):
    for rows, K, tapc in (([10], [48], [0]), ([10], [9 * 48], [48]), ([10], [64], [48]), ([0], [64], [0]),
                          ([1] * 5, [64] * 5, [0] * 5)):
        with pytest.raises(RuntimeError):
            ops.input_proj_x6_plan(rows, K, tapc)
