"""Host checks of the self-attention input builders in tests/helpers.py (``attn_grid_inputs``, ``attn_shift``,
``attn_dominant_keys``): the properties the bitwise assertions of tests/test_gpu_self_attention.py rest on, shown with torch on the
CPU in fp32 against fp64 -- exact scores, exact shifts, a shift-invariant composition, and a dominant key that reproduces its value
row bit for bit.  The deliberately wrong compositions (``attn_compose(drop_tile=, skip_max=)``) are shown to break them."""
import pytest
import torch

import helpers as Hh

SHAPES = [(2, 256, 8), (5, 640, 8), (3, 49, 5)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "B%d-N%d-M%d" % s)
def case(request):
    B, N, M = request.param
    return (B, N, M) + Hh.attn_grid_inputs(1000 + N + M, B, N, M)


def test_grid_values_are_on_the_grid_and_exact_in_bf16(case):
    B, N, M, q, k, v, go = case
    for t in (q, k):
        assert t.shape == (B, N, M * 32) and t.dtype == torch.float32
        assert torch.equal(t * 8, (t * 8).round()) and float(t.abs().max()) <= 1.0
        assert torch.equal(t.bfloat16().float(), t)
    assert bool((q[..., 0::32] == 1).all()) and bool((k[..., 0::32] == 0).all())
    assert len(torch.unique(q)) == 17 and len(torch.unique(k)) == 17          # the whole grid is in use
    assert abs(float(v.std()) - 1) < 0.05 and abs(float(go.std()) - 1) < 0.05
    for c in (96.0, -96.0, Hh.ATTN_DOMINANT):
        assert float(torch.tensor(c).bfloat16()) == c


def test_scores_are_exact_and_the_shift_is_exact(case):
    B, N, M, q, k, v, go = case
    s32 = Hh.attn_scores(q, k, M)
    s64 = Hh.attn_scores(q.double(), k.double(), M)
    assert torch.equal(s32.double(), s64)                                       # fp32 matmul == fp64 matmul
    assert 6 < float(s64.abs().max()) < 16 and 1.9 < float(s64.std()) < 2.3     # max |s| ~ 11, std ~ 2.1
    for c in (96.0, -96.0):
        kc = Hh.attn_shift(k, M, c)
        assert torch.equal(kc[..., 1::32], k[..., 1::32]) and bool((kc[..., 0::32] == c).all())
        assert torch.equal(Hh.attn_scores(q, kc, M), s32 + c)                   # exact in fp32
        assert torch.equal(Hh.attn_scores(q, kc, M).double(), s64 + c)


def test_fp32_composition_is_shift_invariant_bitwise(case):
    B, N, M, q, k, v, go = case
    base = Hh.attn_compose(q, k, v, M)
    ref = Hh.attn_compose(q.double(), k.double(), v.double(), M)
    assert float((base.double() - ref).abs().max()) < 2e-5
    for c in (96.0, -96.0):
        assert torch.equal(Hh.attn_compose(q, Hh.attn_shift(k, M, c), v, M), base)
    # teeth: without the maximum, exp(s) overflows at +96 (inf / inf) and underflows at -96
    for c in (96.0, -96.0):
        assert not torch.equal(Hh.attn_compose(q, Hh.attn_shift(k, M, c), v, M, skip_max=True), base)
    assert not bool(torch.isfinite(Hh.attn_compose(q, Hh.attn_shift(k, M, 96.0), v, M, skip_max=True)).all())


def test_dominant_keys_cover_every_tile_and_select_their_value_row(case):
    B, N, M, q, k, v, go = case
    ntile = (N + 15) // 16
    kd, keys = Hh.attn_dominant_keys(k, B, N, M)
    assert B * M >= ntile and keys.shape == (B, M)
    assert sorted(set((keys // 16).flatten().tolist())) == list(range(ntile))   # every tile is dominant for some (b, h)
    assert int(keys.max()) <= N - 1 and int((kd != k).sum()) == B * M
    for b in range(B):
        for h in range(M):
            t = (b * M + h) % ntile
            assert int(keys[b, h]) == min(16 * t + (5 * t) % 16, N - 1) and float(kd[b, keys[b, h], h * 32]) == 128.0
    s = Hh.attn_scores(q.double(), kd.double(), M)
    top2 = s.topk(2, -1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) > 104                     # every other probability is exactly 0 in fp32
    out = Hh.attn_compose(q, kd, v, M)
    assert Hh.attn_dominant_mismatches(out, v, keys, M) == []
    for b in range(B):
        for h in range(M):
            assert torch.equal(out[b, :, h * 32:(h + 1) * 32], v[b, keys[b, h], h * 32:(h + 1) * 32].expand(N, 32))
    vb = v.bfloat16()
    assert Hh.attn_dominant_mismatches(Hh.attn_compose(q, kd, vb.float(), M).bfloat16(), vb, keys, M) == []
    # teeth: a composition that never sees tile `t` misses exactly the (b, h) whose dominant key lives there
    t = ntile - 1
    bad = Hh.attn_dominant_mismatches(Hh.attn_compose(q, kd, v, M, drop_tile=t), v, keys, M)
    assert bad and all(tt == t for _, _, tt in bad)
    assert len(Hh.attn_dominant_mismatches(Hh.attn_compose(q, kd, v, M, skip_max=True), v, keys, M)) == B * M


def test_rotation_reaches_the_tiles_a_small_batch_leaves_out():
    B, N, M = 1, 33, 1
    q, k, v, go = Hh.attn_grid_inputs(7, B, N, M)
    tiles = set()
    for rot in range(3):
        kd, keys = Hh.attn_dominant_keys(k, B, N, M, rot=rot)
        tiles.add(int(keys[0, 0]) // 16)
        assert Hh.attn_dominant_mismatches(Hh.attn_compose(q, kd, v, M), v, keys, M) == []
    assert tiles == {0, 1, 2}
