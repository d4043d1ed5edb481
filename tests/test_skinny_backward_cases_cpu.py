"""CPU: the cases of tests/test_gpu_skinny_backward.py (tests/skinny_backward_restated.py) are exact in float32, cover the
paths they are named for, and can tell every listed defect from the right answer."""
import pytest
import torch

import skinny_backward_restated as R


def _differs(a, b):
    return any(a[k] is not None and not torch.equal(a[k], b[k]) for k in ("gx", "gw", "gb"))


def test_every_case_is_exact_in_float32():
    assert len({c["name"] for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        R.assert_exact(c, R.inputs(c["M"], c["K"], c["N"]))
    for K in R.FORWARD_K:
        for N in R.FORWARD_N:
            for M in R.FORWARD_M:
                R.assert_exact_forward(*R.forward_inputs(M, K, N), 0.25)


def test_the_expectation_survives_float32_and_an_off_grid_input_is_refused():
    for c in R.CASES:
        if c["M"] in (33, 1025) and (c["K"], c["N"]) in ((256, 256), (64, 192)):
            R.assert_float32_holds(R.expected(c, R.inputs(c["M"], c["K"], c["N"])))
    c = R.CASES[0]
    g, y, x, w, a1, a2 = R.inputs(c["M"], c["K"], c["N"])
    with pytest.raises(AssertionError):
        R.assert_exact(c, (g + 0.1, y, x, w, a1, a2))
    with pytest.raises(AssertionError):   # a denormal in y
        R.assert_exact(c, (g, torch.full_like(y, 1e-40), x, w, a1, a2))


def test_the_cases_reach_the_paths_they_are_named_for():
    ms = {c["M"] for c in R.CASES}
    assert set(R.M_SWEEP) <= ms and max(ms) == R.MAX_M
    # second and later batches of a lane group's share, full and partly filled; the last share empty or short
    rpg = {m: -(-m // R.GROUPS) for m in R.M_SWEEP}
    assert [m for m in R.M_SWEEP if rpg[m] > R.BATCH] == [1025, 1056, 1057, 2048, 2049, 4096]
    assert rpg[1024] == 32 and rpg[1025] == 33 and rpg[1057] == 34 and rpg[2048] == 64 and rpg[2049] == 65 and rpg[4096] == 128
    assert any(R.GROUPS * rpg[m] - m >= rpg[m] for m in R.M_SWEEP)          # a lane group without any row
    # both weight-gradient forms at every M of the sweep, and the boundary between them from both sides
    for K, N in ((256, 256), (256, 1024)):
        assert {c["M"] for c in R.CASES if (c["K"], c["N"]) == (K, N) and c["name"].startswith("sweep")} == set(R.M_SWEEP)
    assert not R.gw32(256, 256) and R.gw32(256, 1024) and R.gw32(1024, 256)
    assert (512 // 16) * (256 // 16) == 512 and not R.gw32(256, 512) and (576 // 16) * (256 // 16) == 576 and R.gw32(256, 576)
    # float4 steps of the gx reduction per lane group: 1 (B4 = 1), 2 (B4 = 2), 3 and 9 (B4 = 1, several trips), 4 and 16 (B4 = 4)
    assert {N // 64 for K, N in R.WEIGHT_SHAPES} | {4, 16} == {1, 2, 3, 4, 8, 9, 16}
    for opt in R.OPTIONS:
        for relu in ("relu", "norelu"):
            assert sum(c["name"].startswith(opt + "-M") and c["name"].endswith("-" + relu) for c in R.CASES) == 4, (opt, relu)


@pytest.mark.parametrize("name", [d[0] for d in R.DEFECTS])
def test_a_case_resolves_the_defect(name):
    shows = dict(R.DEFECTS)[name]
    tried = []
    for c in sorted((c for c in R.CASES if shows(c)), key=lambda c: c["M"] * (c["K"] + c["N"])):
        inp = R.inputs(c["M"], c["K"], c["N"])
        good, bad = R.expected(c, inp), R.expected(c, inp, defect=name)
        tried.append(c["name"])
        if _differs(good, bad):
            print(f"defect '{name}': resolved by case {c['name']}")
            R.assert_float32_holds(good)
            return
        if len(tried) >= 8:
            break
    assert False, f"defect '{name}': no case among {tried} has an expectation that differs"


def test_a_defect_leaves_the_cases_it_cannot_show_at_alone():
    """The predicates of DEFECTS are not vacuous the other way: where one says the defect cannot show, the expectation is the
    right one (checked at the small shapes)."""
    for name, shows in R.DEFECTS:
        for c in R.CASES:
            if not shows(c) and c["M"] <= 33 and c["K"] * c["N"] <= 256 * 256:
                inp = R.inputs(c["M"], c["K"], c["N"])
                assert not _differs(R.expected(c, inp), R.expected(c, inp, defect=name)), (name, c["name"])


def test_forward_statement():
    x, w, b = R.forward_inputs(17, 64, 33)
    want = torch.relu((x.double() @ w.double().t() + b.double()) * 0.25)
    assert torch.equal(R.expected_forward(x, w, b, 0.25, True), want) and bool((want.float().double() == want).all())
