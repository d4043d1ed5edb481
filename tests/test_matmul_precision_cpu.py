"""CPU: the opt-in bf16 matmul precision of the training token GEMMs (egtr_amd.ops.set_matmul_precision) -- the
switch itself, the trainer argument, the host restatement of the one-piece weight stream, and the operands, reference, bar and
teeth that tests/test_gpu_matmul_precision.py runs the kernels against (stated here so that they are checked without a GPU).

Reference and bar.  The one-term kernels multiply RNE(a) by RNE(w) and accumulate in fp32; every bf16 x bf16 product is exact in
fp32, so against the float64 product of the ROUNDED operands the only error left is the fp32 accumulation of K terms:
|got - ref| <= 2 K 2^-24 sum_k |a_r w_r| per element (the standard summation bound, doubled for the matrix unit's unspecified
internal order; K is the reduced length, M for a weight gradient).  An O(1) epilogue addend (bias, add1, add2) enters with one
fp32 rounding of the value it produces.

Teeth.  ``operand`` draws one-sign values that sit a known fraction of a bf16 ulp above a bf16 value: a quarter of them 0.05-0.45
ulp above (RNE and truncation both round down), three quarters 0.55-0.95 ulp above (RNE rounds up, truncation down).  Against
the RNE product, the truncated product is then low by ~0.75 ulp per operand and element, the exact fp32 product off by
~0.125 ulp per operand and element in one direction, and a dropped 16-wide k-step removes 16 / K of a one-sign sum: all three
far outside a bar of 2 K 2^-24 relative for K up to several thousand, which ``assert_teeth`` checks on every input used."""
import pytest
import torch

U = 2.0 ** -24


# ---- operands, reference, bar, teeth (shared with the GPU tests) --------------------------------------------------------------
def operand(shape, seed, scale=1.0):
    """fp32, all positive: (1 + (m + f) 2^-7) 2^e scale with m in 0..127, e in {-1, 0, 1} and f the fraction of a bf16 ulp the
    value lies above the bf16 value below it: 0.05-0.45 for a quarter of the elements, 0.55-0.95 for the rest (multiples of
    2^-10, so the value has 18 significant bits and is exact in fp32).  ``scale``: a power of two."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 128, shape, generator=g).double()
    low = torch.rand(shape, generator=g) < 0.25
    f = torch.randint(0, 410, shape, generator=g).double() / 1024 + torch.where(low, 0.05, 0.55)
    f = (f * 1024).round() / 1024
    e = torch.randint(-1, 2, shape, generator=g).double()
    v = (1.0 + (m + f) / 128) * torch.pow(2.0, e) * scale
    out = v.float()
    assert torch.equal(out.double(), v)
    return out


def rne(t):
    """fp32 -> the fp32 value of its bf16 rounding (torch's cast rounds to nearest even)"""
    return t.to(torch.bfloat16).float()


def trunc(t):
    """fp32 -> the fp32 value of its upper 16 bits"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def product_ref(a, w):
    """(float64 product of the RNE-rounded operands a [M, K], w [N, K], the bar 2 K 2^-24 sum |a_r w_r|) per element"""
    ar, wr = rne(a).double(), rne(w).double()
    K = a.shape[1]
    return ar @ wr.t(), 2.0 * K * U * (ar.abs() @ wr.abs().t())


def assert_teeth(a, w):
    """The bar separates the one-term RNE product of (a, w) from its three nearest wrong neighbours in at least half of the
    output elements: truncated operands, unrounded operands, one 16-wide k-step dropped."""
    ref, bar = product_ref(a, w)
    K = a.shape[1]
    ar, wr = rne(a).double(), rne(w).double()
    wrong = {"truncated operands": trunc(a).double() @ trunc(w).double().t(),
             "unrounded operands (the switch ignored)": a.double() @ w.double().t(),
             "one k-step dropped": ref - ar[:, K - 16:] @ wr[:, K - 16:].t()}
    for name, v in wrong.items():
        share = ((v - ref).abs() > bar).double().mean().item()
        assert share >= 0.5, (name, share, tuple(a.shape), tuple(w.shape))


def stream_definition(w):
    """The one-piece weight stream from its definition: block (n / 128, k / 32) holds rows n % 128, columns k % 32 of RNE(w)"""
    N, K = w.shape
    out = torch.empty(N // 128, K // 32, 128, 32, dtype=torch.bfloat16)
    wb = w.to(torch.bfloat16)
    for nb in range(N // 128):
        for kb in range(K // 32):
            out[nb, kb] = wb[nb * 128:(nb + 1) * 128, kb * 32:(kb + 1) * 32]
    return out


FORWARD_SHAPES = [(M, K, N) for M in (37, 200) for K in (32, 64, 256, 1024) for N in (128, 384)]
WGRAD_SHAPES = [(200, 128, 128), (4133, 256, 128), (4133, 128, 1024)]


# ---- the switch -----------------------------------------------------------------------------------------------------------
def test_switch_default_set_get_context_manager_and_bad_values():
    from egtr_amd import ops
    assert "EGTR_MATMUL_PRECISION" in ops.ENV_ROUTE_SWITCHES
    before = ops.matmul_precision()
    try:
        ops.set_matmul_precision("fp32")
        assert ops.matmul_precision() == "fp32" and ops.MATMUL_PRECISION == "fp32"
        assert ops.set_matmul_precision("bf16") == "fp32" and ops.matmul_precision() == "bf16" and ops.MATMUL_PRECISION == "bf16"
        assert ops.set_matmul_precision("fp32") == "bf16" and ops.matmul_precision() == "fp32"
        with ops.matmul_precision_mode("bf16"):
            assert ops.matmul_precision() == "bf16"
            with ops.matmul_precision_mode("fp32"):
                assert ops.matmul_precision() == "fp32"
            assert ops.matmul_precision() == "bf16"
        assert ops.matmul_precision() == "fp32"
        with pytest.raises(KeyError):
            with ops.matmul_precision_mode("bf16"):
                raise KeyError("x")
        assert ops.matmul_precision() == "fp32"                      # restored on the way out of an exception too
        for bad in ("fp16", "BF16", 16, None, ""):
            with pytest.raises(ValueError):
                ops.set_matmul_precision(bad)
            with pytest.raises(ValueError):
                ops.matmul_precision_mode(bad)
        assert ops.matmul_precision() == "fp32"                      # a refused value changes nothing
    finally:
        ops.set_matmul_precision(before)


def test_default_is_fp32_and_the_environment_variable_is_read_and_checked_at_import():
    """A fresh interpreter: no variable -> "fp32"; "bf16" -> "bf16"; anything else raises ValueError at import."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from egtr_amd import ops; print(ops.matmul_precision(), ops._gemm_terms())"

    def run(value):
        env = {k: v for k, v in os.environ.items() if k != "EGTR_MATMUL_PRECISION"}
        if value is not None:
            env["EGTR_MATMUL_PRECISION"] = value
        return subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)

    r = run(None)
    assert r.returncode == 0 and r.stdout.split() == ["fp32", "6"], r.stderr
    r = run("bf16")
    assert r.returncode == 0 and r.stdout.split() == ["bf16", "1"], r.stderr
    r = run("16")
    assert r.returncode != 0 and "ValueError" in r.stderr


def test_torch_matmul_precision_is_neither_read_nor_set():
    from egtr_amd import ops
    before, ambient = torch.get_float32_matmul_precision(), ops.matmul_precision()
    try:
        with ops.matmul_precision_mode("bf16"):
            assert torch.get_float32_matmul_precision() == before
        for theirs in ("medium", "highest"):
            torch.set_float32_matmul_precision(theirs)
            assert ops.matmul_precision() == ambient and ops._gemm_terms() == (1 if ambient == "bf16" else 6)
    finally:
        torch.set_float32_matmul_precision(before)


def test_trainer_argument_enters_and_leaves_the_mode():
    """DataParallelTrainer(matmul_precision=...): every training_step runs inside the context manager; None follows the global
    setting; a bad value raises at construction.  A stand-in model on CPU tensors records the mode it ran under."""
    from egtr_amd import ops
    from egtr_amd.runtime import DataParallelTrainer
    seen = []

    class _Out:
        def __init__(self, loss):
            self.loss, self.loss_dict = loss, {}

    class _M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, pixel_values, pixel_mask, labels, **kw):
            seen.append(ops.matmul_precision())
            return _Out((self.w * pixel_values.sum()).sum())

    batch = {"pixel_values": torch.ones(1, 3, 4, 4), "pixel_mask": torch.ones(1, 4, 4, dtype=torch.long), "labels": []}
    before = ops.set_matmul_precision("fp32")
    try:
        for arg, ambient, want in (("bf16", "fp32", "bf16"), ("fp32", "bf16", "fp32"), (None, "fp32", "fp32"),
                                   (None, "bf16", "bf16")):
            m = _M()
            tr = DataParallelTrainer(m, optimizer=torch.optim.SGD(m.parameters(), lr=0.1), accumulate=1,
                                     matmul_precision=arg)
            ops.set_matmul_precision(ambient)
            _, _, stepped = tr.training_step(batch)
            assert stepped and seen[-1] == want, (arg, ambient, seen[-1])
            assert ops.matmul_precision() == ambient, "the trainer must leave the global setting as it found it"
            assert float(m.w.detach()) != 1.0
        with pytest.raises(ValueError):
            DataParallelTrainer(_M(), optimizer=torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1),
                                matmul_precision="fp16")
        tr = DataParallelTrainer(_M(), optimizer=torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1),
                                 matmul_precision="bf16", deterministic=True)      # the two modes combine
        ops.set_matmul_precision("fp32")
        tr.training_step(batch)
        assert seen[-1] == "bf16" and ops.matmul_precision() == "fp32"
    finally:
        ops.set_matmul_precision(before)


# ---- the one-piece weight stream ------------------------------------------------------------------------------------------
def test_one_piece_weight_stream_restatement_against_its_definition():
    from egtr_amd import ops
    w = operand((256, 96), 5)
    w[3, 7] = float("inf")
    w[130, 40] = float("nan")
    w[0, 0] = 3.0e38            # finite, between the largest bf16 (3.3895e38) and its upper rounding boundary: stays finite
    w[0, 1] = 3.4e38            # finite, beyond the boundary: rounds to inf (documented)
    s = ops.gemm_split_weights(w, terms=1)
    assert s.dtype == torch.bfloat16 and tuple(s.shape) == (2, 3, 128, 32) and s.is_contiguous()
    assert torch.equal(s.view(torch.int16), stream_definition(w).view(torch.int16))
    assert torch.isinf(s[0, 0, 3, 7]) and torch.isnan(s[1, 1, 2, 8])
    assert torch.isfinite(s[0, 0, 0, 0]) and torch.isinf(s[0, 0, 0, 1])
    # rounding is to nearest EVEN: 1 + 2^-8 lies half way between the bf16 values 1 and 1 + 2^-7
    t = torch.full((128, 32), 1.0 + 2.0 ** -8)
    t[0, 1] = 1.0 + 2.0 ** -7 + 2.0 ** -8      # half way between an odd and an even bf16 value: up
    st = ops.gemm_split_weights(t, terms=1).float()
    assert st[0, 0, 0, 0] == 1.0 and st[0, 0, 0, 1] == 1.0 + 2.0 ** -6
    # the six-term stream is what it was, and the two are told apart by their shape
    assert tuple(ops.gemm_split_weights(w[:, :64]).shape) == (2, 2, 3, 128, 32)
    with pytest.raises(ValueError):
        ops.gemm_split_weights(w, terms=3)


@pytest.mark.parametrize("M,K,N", FORWARD_SHAPES)
def test_bar_separates_the_one_term_product_from_its_wrong_neighbours_forward(M, K, N):
    assert_teeth(operand((M, K), 11), operand((N, K), 12, scale=1.0 / 16))


@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
def test_bar_separates_the_one_term_product_from_its_wrong_neighbours_wgrad(M, N, K):
    """the weight gradient g^T x is the product of g^T [N, M] and x^T [K, M]: reduced length M"""
    g, x = operand((M, N), 13, scale=1.0 / 16), operand((M, K), 14)
    assert_teeth(g.t().contiguous(), x.t().contiguous())
