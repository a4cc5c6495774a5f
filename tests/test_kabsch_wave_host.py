"""The lane form of the Kabsch solve (csrc/kabsch_wave.hpp) by the host's lane group — pcr_kabsch_solve_lanes, the text a wavefront runs
on the device — against the scalar form (pcr_kabsch_solve, csrc/numerics.hpp): the same return code and the same BITS of R and t on every case; nothing
is compared with a tolerance.  The host's lane group also checks every vote of the step (the branches a wavefront takes as one): lanes that disagree make
the call return PCR_ERR_STATE, which no scalar solve returns.  No GPU.  The cases (kabsch_wave_cases.py): one or more of every class the solve branches on, by construction, and
20 000 seeded ones."""
import numpy as np
import pytest

import kabsch_wave_cases as cases


def both(pcr, sums):
    rs, Rs, ts = pcr.kabsch_solve(sums)
    rl, Rl, tl = pcr.kabsch_solve_lanes(sums)
    return (rs, Rs.view(np.uint32).tobytes(), ts.view(np.uint32).tobytes()), (rl, Rl.view(np.uint32).tobytes(), tl.view(np.uint32).tobytes()), (Rs, ts)


@pytest.fixture(scope="module")
def constructed(synth):
    return cases.constructed(synth)


def test_constructed_classes(pcr, constructed):
    names = [n for n, _ in constructed]
    for want in ("real correspondences", "diagonal", "permutation (1, 2, 0)", "identity multiple", "rank 2", "rank 1", "H == 0", "reflection", "M = 0", "M = 1",
                 "scene x 0.001", "scene x 1e+06", "1 000 m from the origin"):
        assert want in names, want
    for name, sums in constructed:
        s, l, (R, t) = both(pcr, sums)
        # the scalar form itself: 0 or "no pair kept", and numbers — a case is only relied on with that confirmed
        assert s[0] == (cases.ERR_EMPTY if name.startswith("M = 0") else 0), (name, s[0])
        assert np.isfinite(R).all() and np.isfinite(t).all(), name
        if s[0] == 0:
            assert abs(abs(np.linalg.det(R.astype(np.float64))) - 1.0) < 1e-5, name        # (a rotation came out: the repairs ran where they had to)
        assert l == s, name


def test_branches_are_reached(pcr, constructed):
    """the classes land where they are meant to: the reflection cases have det(U V^T) < 0 (R comes out proper all the same), the rank cases a zero
    singular value — read off numpy's SVD of the H the solve forms"""
    for name, sums in constructed:
        M = sums[15]
        if M <= 0:
            continue
        H = sums[6:15].reshape(3, 3) - M * np.outer(sums[3:6] / M, sums[0:3] / M)
        U, S, Vt = np.linalg.svd(H)
        if name.startswith(("reflection", "mirrored")):
            assert np.linalg.det(U @ Vt) < 0, name
        if name.startswith("rank 2"):
            assert S[1] > 1e-3 * S[0] and S[2] < 1e-12 * S[0], (name, S)
        if name.startswith("rank 1"):
            assert S[0] > 0 and S[1] < 1e-12 * S[0], (name, S)
        if name == "H == 0":
            assert S[0] == 0.0


def test_seeded_cases(pcr):
    sums = cases.seeded(20000)
    n_empty = 0
    for i in range(sums.shape[0]):
        s, l, _ = both(pcr, sums[i])
        assert l == s, (i, sums[i].tolist())
        n_empty += s[0] != 0
    assert n_empty == 0                                 # (every seeded case has a pair)
