"""Cost matrices shared by tests/test_matcher_large_cpu.py (restated solver against scipy) and
tests/test_gpu_matcher_large.py (egtr_hungarian_match_large_f32 against scipy): [N, T] float32, N queries, T targets."""
import numpy as np


def generic(N, T, seed=None):
    rng = np.random.default_rng(1000 * T + N if seed is None else seed)
    return rng.standard_normal((N, T)).astype(np.float32)


def tied_integers(N, T, high, duplicate_lower_half=False):
    """Integer costs in [0, high): exact ties in every scan; optionally the lower half of the queries repeats the upper."""
    rng = np.random.default_rng(7 * N + T + high)
    c = rng.integers(0, high, (N, T)).astype(np.float32)
    if duplicate_lower_half:
        c[N // 2:] = c[:N - N // 2]
    return c


def all_equal(N, T, value=0.25):
    return np.full((N, T), value, dtype=np.float32)


def padded_tokens(N, T):
    """Costs in {0, 1}; the upper half of the queries are identical copies of ONE query -- what padded encoder tokens give in
    the real model (equal logits, box (1, 1, 1, 1))."""
    rng = np.random.default_rng(N + T)
    c = rng.integers(0, 2, (N, T)).astype(np.float32)
    c[N // 2:] = c[N // 2]
    return c


# (id, builder): the tie cases of both test files
TIE_CASES = [
    ("int3_1100x5", lambda: tied_integers(1100, 5, 3)),
    ("int4_1100x5", lambda: tied_integers(1100, 5, 4)),
    ("int3_2500x40", lambda: tied_integers(2500, 40, 3)),
    ("int4_2500x40", lambda: tied_integers(2500, 40, 4)),
    ("equal_1500x7", lambda: all_equal(1500, 7)),
    ("padded_1500x64", lambda: padded_tokens(1500, 64)),
]
# tied integer costs with the lower half of the rows duplicated
DUPLICATED_CASES = [
    ("dup_1100x5", lambda: tied_integers(1100, 5, 3, True)),
    ("dup_2500x40", lambda: tied_integers(2500, 40, 4, True)),
    ("dup_1500x64", lambda: tied_integers(1500, 64, 2, True)),
    ("dup_70x5", lambda: tied_integers(70, 5, 3, True)),
]
