"""CPU: the pieces of the deterministic mode that need no GPU -- the fixed-point helpers of csrc/fixed_accum.h (a stand-alone
host program built with the sanitizers), the switch in ``egtr_amd.ops``, and the numpy restatement of the relation loss's tie
rule that tests/test_gpu_deterministic.py compares the kernels with."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixed_accum_header_under_sanitizers(tmp_path):
    """tests/fixed_accum_check.cpp: no overflow at the worst case of the bound (both signs, up to 2^40 terms), one bit pattern
    over 50 random orders of one list of contributions, exact scaling by 2^+-40 -- compiled with the host compiler and
    -fsanitize=undefined,address, run directly."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fixed_accum_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "egtr_amd", "csrc"), os.path.join(ROOT, "tests", "fixed_accum_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fixed_accum ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_switch_follows_both_sources_and_the_context_manager_restores():
    from egtr_amd import ops
    assert "EGTR_DETERMINISTIC" in ops.ENV_ROUTE_SWITCHES
    before, torch_before = ops.DETERMINISTIC, torch.are_deterministic_algorithms_enabled()
    try:
        ops.set_deterministic(False)
        torch.use_deterministic_algorithms(False)
        assert ops.is_deterministic() is False
        assert ops.set_deterministic(True) is False and ops.is_deterministic() is True and ops.DETERMINISTIC is True
        assert ops.set_deterministic(False) is True and ops.is_deterministic() is False
        torch.use_deterministic_algorithms(True, warn_only=True)      # torch's own switch is honoured ...
        assert ops.is_deterministic() is True and ops.DETERMINISTIC is False   # ... and never set from here
        torch.use_deterministic_algorithms(False)
        assert ops.is_deterministic() is False
        with ops.deterministic():
            assert ops.is_deterministic() is True
            with ops.deterministic(False):
                assert ops.is_deterministic() is False
            assert ops.is_deterministic() is True
        assert ops.is_deterministic() is False and ops.DETERMINISTIC is False
        assert torch.are_deterministic_algorithms_enabled() is False        # the mode never touched torch's switch
        with pytest.raises(KeyError):
            with ops.deterministic():
                raise KeyError("x")
        assert ops.DETERMINISTIC is False                                   # restored on the way out of an exception too
    finally:
        ops.set_deterministic(before)
        torch.use_deterministic_algorithms(torch_before)


def test_float64_backward_is_refused_by_name_under_the_mode():
    """The check sits in front of any device work, so it is visible without a GPU."""
    from egtr_amd import ops
    from egtr_amd.load_custom import _MultiScaleDeformableAttention as K
    v = torch.zeros(1, 5, 2, 4, dtype=torch.float64)
    shp = torch.tensor([[1, 5]])
    lsi = torch.tensor([0])
    loc = torch.zeros(1, 3, 2, 1, 2, 2, dtype=torch.float64)
    at = torch.zeros(1, 3, 2, 1, 2, dtype=torch.float64)
    with ops.deterministic():
        with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
            K.ms_deform_attn_backward(v, shp, lsi, loc, at, torch.zeros(1, 3, 8, dtype=torch.float64), 64)


# ---- the tie rule of egtr_relation_loss_f32 with deterministic = 1: restated with numpy ------------------------------------
# (tests/loss_restated.py; tests/test_gpu_deterministic.py imports the two names from here)
from loss_restated import relation_selection, topk_lowest_index_first  # noqa: E402,F401


def test_tie_rule_restatement():
    x = np.array([[0.5, 0.0, 0.5], [0.5, -0.5, 0.5]], dtype=np.float32)
    cand = np.array([[1, 1, 0], [1, 1, 1]], dtype=bool)
    assert topk_lowest_index_first(x, cand, 2).tolist() == [[True, False, False], [True, False, False]]
    assert topk_lowest_index_first(x, cand, 4).tolist() == [[True, True, False], [True, False, True]]
    assert not topk_lowest_index_first(x, cand, 0).any()
    assert (topk_lowest_index_first(x, cand, 9) == cand).all()
