"""The backward of the skinny linear layer (csrc/linear.hip: egtr_linear_backward_acc_f32) and its forward (egtr_linear_f32)
stated in float64 with torch tensor ops, apart from the kernels:

    g' = alpha * g * [y > 0]          (y: the layer's post-ReLU output, optional)
    gx = g' W (+ add1) (+ add2)       [M, K]
    gw = g'^T x                       [N, K]
    gb = column sums of g'            [N]

together with GRID INPUTS on which every sum of every summation order is exactly representable in float32 -- g, x, W multiples
of 1/4 in [-2, 2], the addends multiples of 1/16 in [-4, 4], alpha 1 or 1/4: with M <= 4096 and N, K <= 1024 every partial sum
is a multiple of 1/64 below 2^15, 21 bits (``assert_exact``) -- so the GPU test (tests/test_gpu_skinny_backward.py) asserts
equality, not a tolerance; the cases of that test; and ``DEFECTS``: deliberately wrong restatements that mimic what the kernel
could get wrong (its weight-gradient tiles split the M rows over 32 lane groups, ceil(M / 32) rows each, walked in batches of
32).  tests/test_skinny_backward_cases_cpu.py shows that the cases resolve every defect.  Not a test module."""
import functools

import numpy as np
import torch

GROUPS, BATCH = 32, 32                     # lane groups a weight-gradient tile splits the rows over; rows per load batch
MAX_M, MAX_NK = 4096, 1024
M_SWEEP = (1, 15, 16, 17, 31, 32, 33, 800, 1023, 1024, 1025, 1056, 1057, 2048, 2049, 4096)
WEIGHT_SHAPES = ((64, 64), (64, 128), (64, 192), (256, 512), (256, 576), (1024, 256))       # (K, N)
OPTIONS = ("plain", "add1", "add2", "both", "alias-add1", "alias-add2", "no-gb", "no-gx", "no-gw", "alpha-quarter")


def gw32(K, N):
    """The 32 x 32 weight-gradient form: more than 512 tiles of 16 x 16."""
    return (N // 16) * (K // 16) > 512


def case(M, K, N, relu=True, add1=False, add2=False, alias=None, want_gx=True, want_gw=True, want_gb=True, alpha=1.0, tag=""):
    name = f"{tag}-M{M}-K{K}-N{N}-{'relu' if relu else 'norelu'}"
    return dict(name=name, M=M, K=K, N=N, relu=relu, add1=add1, add2=add2, alias=alias, want_gx=want_gx, want_gw=want_gw,
                want_gb=want_gb, alpha=alpha)


def _option(opt, M, K, N, relu):
    kw = {"plain": {}, "add1": dict(add1=True), "add2": dict(add2=True), "both": dict(add1=True, add2=True),
          "alias-add1": dict(add1=True, alias="add1"), "alias-add2": dict(add1=True, add2=True, alias="add2"),
          "no-gb": dict(add1=True, want_gb=False), "no-gx": dict(want_gx=False), "no-gw": dict(add1=True, want_gw=False),
          "alpha-quarter": dict(add1=True, add2=True, alpha=0.25)}[opt]
    return case(M, K, N, relu=relu, tag=opt, **kw)


def _cases():
    out = []
    for K, N in ((256, 256), (256, 1024)):        # 16 x 16 form with four float4 steps per batch; 32 x 32 form (fc1's backward)
        for M in M_SWEEP:
            out.append(case(M, K, N, relu=True, add1=True, tag="sweep"))
    for K, N in WEIGHT_SHAPES:
        for M in (33, 1025):
            out.append(case(M, K, N, relu=True, tag="shape"))
    for K, N in ((256, 256), (256, 1024)):
        for M in (33, 1025):
            for opt in OPTIONS:
                for relu in (True, False):
                    out.append(_option(opt, M, K, N, relu))
    return out


CASES = _cases()
CONTAINMENT = (1057, 256, 256)
INEXACT = (1025, 256, 256)
FORWARD_K, FORWARD_N, FORWARD_M = (64, 256, 320, 512, 1024), (2, 33, 256), (1, 17, 1025)


# ------------------------------------------------------------------------------------------------------------------- inputs
def _grid(rng, shape, step, bound):
    """Multiples of ``step`` in [-bound, bound], float32."""
    n = int(round(bound / step))
    return torch.from_numpy((rng.integers(-n, n + 1, size=shape) * step).astype(np.float32))


@functools.lru_cache(maxsize=3)
def inputs(M, K, N):
    """(g [M, N], y [M, N], x [M, K], w [N, K], add1 [M, K], add2 [M, K]) on their grids, CPU float32; the same tensors for every
    case of a shape (never written to).  y: about half positives (multiples of 1/4 in (0, 2]), the rest zeros, every third of
    them -0.0; no denormals."""
    rng = np.random.Generator(np.random.PCG64(7_000_000 + 4099 * M + 17 * K + N))
    g, x, w = _grid(rng, (M, N), 0.25, 2.0), _grid(rng, (M, K), 0.25, 2.0), _grid(rng, (N, K), 0.25, 2.0)
    a1, a2 = _grid(rng, (M, K), 1 / 16, 4.0), _grid(rng, (M, K), 1 / 16, 4.0)
    pos = torch.from_numpy((rng.integers(1, 9, size=(M, N)) * 0.25).astype(np.float32))
    kind = torch.from_numpy(rng.integers(0, 6, size=(M, N)))                   # 0..2 positive, 3..4 zero, 5 negative zero
    y = torch.where(kind < 3, pos, torch.zeros_like(pos))
    y = torch.where(kind == 5, torch.full_like(pos, -0.0), y)
    return g, y, x, w, a1, a2


def forward_inputs(M, K, N):
    """(x [M, K], w [N, K], b [N]) on the grids."""
    rng = np.random.Generator(np.random.PCG64(9_000_000 + 4099 * M + 17 * K + N))
    return _grid(rng, (M, K), 0.25, 2.0), _grid(rng, (N, K), 0.25, 2.0), _grid(rng, (N,), 1 / 16, 4.0)


def _on_grid(t, step, bound):
    v = t.double() / step
    return t.dtype == torch.float32 and bool((v == v.round()).all()) and float(t.abs().max()) <= bound


def assert_exact(c, inp):
    """Every partial sum of every summation order of the case is a multiple of 1/64 below 2^15: exactly representable in
    float32 (24 bits), so the float64 statement is what ANY correct float32 evaluation gives, bit for bit."""
    g, y, x, w, a1, a2 = inp
    M, K, N = c["M"], c["K"], c["N"]
    assert tuple(g.shape) == (M, N) and tuple(x.shape) == (M, K) and tuple(w.shape) == (N, K) and tuple(y.shape) == (M, N)
    assert 1 <= M <= MAX_M and K <= MAX_NK and N <= MAX_NK and K % 64 == 0 and N % 64 == 0
    assert all(_on_grid(t, 0.25, 2.0) for t in (g, x, w)) and all(_on_grid(t, 1 / 16, 4.0) for t in (a1, a2))
    assert c["alpha"] in (1.0, 0.25)
    # products are multiples of 1/16; a sum of n of them is below 4 n; alpha = 1/4 makes it a multiple of 1/64
    largest = 4.0 * max(M, N) + 8.0
    assert largest < 2.0 ** 15 and (2.0 ** 15) * 64 <= 2.0 ** 24
    # y: exact zeros of both signs and positives, nothing denormal
    tiny = torch.finfo(torch.float32).tiny
    assert bool(((y == 0) | (y >= tiny)).all())
    if M * N >= 64:
        frac = float((y > 0).double().mean())
        assert 0.3 < frac < 0.7
        assert bool((torch.signbit(y) & (y == 0)).any()) and bool((~torch.signbit(y) & (y == 0)).any())


def assert_exact_forward(x, w, b, alpha):
    assert _on_grid(x, 0.25, 2.0) and _on_grid(w, 0.25, 2.0) and _on_grid(b, 1 / 16, 4.0) and alpha in (1.0, 0.25)
    assert 4.0 * x.shape[1] + 4.0 < 2.0 ** 15


# ---------------------------------------------------------------------------------------------------------------- reference
def _share(M):
    """For every row: its index inside its lane group's share of ceil(M / 32) rows."""
    rpg = (M + GROUPS - 1) // GROUPS
    return torch.arange(M) % rpg, rpg


def expected(c, inp, defect=None, alpha=None):
    """{"gx", "gw", "gb"} in float64 (None for an output the case does not ask for), on the device of the inputs.  ``defect``
    names one deliberate mistake (see DEFECTS).  ``alpha`` overrides the case's (the inexact case)."""
    g, y, x, w, a1, a2 = (t.double() for t in inp)
    M, K, N = c["M"], c["K"], c["N"]
    alpha = c["alpha"] if alpha is None else alpha
    dev = g.device
    if c["relu"]:
        mask = (y >= 0) if defect == "mask taken as y >= 0" else (y > 0)
        gm = g * mask.to(g.dtype)
    else:
        gm = g
    gp = alpha * gm
    gx = gp @ w
    add_scale = alpha if defect == "alpha applied to the addends" else 1.0
    if c["add1"]:
        gx = gx + add_scale * a1
    if c["add2"] and defect != "add2 ignored":
        gx = gx + add_scale * a2
    # the weight-side reductions run over the rows
    rows = torch.ones(M, dtype=g.dtype, device=dev)
    idx, rpg = _share(M)
    if defect == "rows of a share beyond its first 32 dropped":
        rows = (idx < BATCH).to(g.dtype).to(dev)
    if defect == "last row of each share dropped":
        rows = (idx != rpg - 1).to(g.dtype).to(dev)
    if defect == "rows past M added as copies of row M - 1":
        rows = rows.clone()
        rows[M - 1] += GROUPS * rpg - M
    gr = gp * rows[:, None]
    gw = gr.t() @ x
    gb_src = gr
    if defect == "mask ignored in gb":
        gb_src = alpha * g * rows[:, None]
    gb = gb_src.sum(0)
    if defect == "alpha missing from gb" and alpha != 0:
        gb = gb / alpha
    tile = 32 if gw32(K, N) else 16
    if defect == "gb taken from the wrong column tile":
        gb = gb.roll(tile)
    if defect == "halves of a 32 x 32 tile swapped" and gw32(K, N):
        gw = gw.view(N // 32, 2, 16, K).flip(1).reshape(N, K)
    return dict(gx=gx if c["want_gx"] else None, gw=gw if c["want_gw"] else None, gb=gb if c["want_gb"] else None)


def expected_forward(x, w, b, alpha, relu):
    y = (x.double() @ w.double().t() + b.double()) * alpha
    return torch.relu(y) if relu else y


def assert_float32_holds(ref):
    """The float64 expectation survives the trip through float32: what assert_exact promises, checked on the result."""
    for k, t in ref.items():
        assert t is None or bool((t.float().double() == t).all()), k


# ------------------------------------------------------------------------------------------------------------------ defects
def _rows_any(c):
    return c["want_gw"] or c["want_gb"]


# (name, case -> whether the defect can show at that case)
DEFECTS = [
    ("rows of a share beyond its first 32 dropped", lambda c: c["M"] > GROUPS * BATCH and _rows_any(c)),
    ("last row of each share dropped", _rows_any),
    ("rows past M added as copies of row M - 1", lambda c: c["M"] % GROUPS != 0 and _rows_any(c)),
    ("mask taken as y >= 0", lambda c: c["relu"]),
    ("mask ignored in gb", lambda c: c["relu"] and c["want_gb"]),
    ("alpha missing from gb", lambda c: c["alpha"] != 1.0 and c["want_gb"]),
    ("alpha applied to the addends", lambda c: c["alpha"] != 1.0 and c["want_gx"] and (c["add1"] or c["add2"])),
    ("add2 ignored", lambda c: c["add2"] and c["want_gx"]),
    ("gb taken from the wrong column tile", lambda c: c["want_gb"]),
    ("halves of a 32 x 32 tile swapped", lambda c: c["want_gw"] and gw32(c["K"], c["N"])),
]
