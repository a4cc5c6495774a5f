"""The moment sets (16 f64 each: sum p, sum q, sum q p^T row-major, count) that test_kabsch_wave_host.py and test_kabsch_wave_gpu.py put through the
scalar Kabsch solve and its lane form (csrc/kabsch_wave.hpp).  Not a test module.  constructed(synth) names each class the solve branches on; seeded(n)
is the random bulk.  With sum p = sum q = 0 the solve's H is sums[6:15] itself, whatever the count: that is how an H is placed exactly."""
import numpy as np

ERR_EMPTY = -6        # PCR_ERR_EMPTY (include/pcr.h)


def moments(p, q):
    """p, q: (n, 3) -> the 16 sums of the pairs (p_i, q_i) in f64"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    return np.concatenate([p.sum(0), q.sum(0), (q[:, :, None] * p[:, None, :]).sum(0).reshape(9), [float(p.shape[0])]])


def from_h(H, count=100.0):
    return np.concatenate([np.zeros(6), np.asarray(H, np.float64).reshape(9), [count]])


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def nearest_pairs(src, tgt, max_corr):
    """(p, q) of the kept correspondences of one ICP iteration: every source point with its nearest target point, squared distance below max_corr"""
    s, t = src.T.astype(np.float64), tgt.T.astype(np.float64)
    d2 = (s * s).sum(1)[:, None] - 2.0 * (s @ t.T) + (t * t).sum(1)[None, :]
    j = d2.argmin(1)
    keep = d2[np.arange(s.shape[0]), j] < max_corr
    return s[keep], t[j[keep]]


def constructed(synth):
    """[(name, sums)]: one or more sets of every class"""
    rng = np.random.default_rng(20240611)
    out = []
    src, tgt = synth.kitti_like_pair(4096)
    p, q = nearest_pairs(src, tgt, 1.0)
    assert p.shape[0] > 1000
    out.append(("real correspondences", moments(p, q)))
    # gamma == 0 exits: H exactly diagonal, exactly a permutation matrix
    out.append(("diagonal", from_h(np.diag([3.0, 2.0, 1.0]))))
    out.append(("diagonal, unsorted", from_h(np.diag([1.0, 3.0, 2.0]))))
    out.append(("diagonal, negative entry", from_h(np.diag([2.0, -3.0, 1.0]))))
    for perm in ((1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (2, 1, 0)):
        out.append((f"permutation {perm}", from_h(np.eye(3)[list(perm)])))
    # tied singular values keep their column order
    out.append(("identity multiple", from_h(2.5 * np.eye(3))))
    out.append(("identity", from_h(np.eye(3))))
    out.append(("two tied", from_h(np.diag([2.0, 2.0, 1.0]))))
    # the three repair branches
    u1, v1, u2, v2 = np.array([1.0, 2.0, -2.0]), np.array([3.0, -1.0, 2.0]), np.array([2.0, 1.0, 2.0]), np.array([1.0, 4.0, 1.0])
    out.append(("rank 2", from_h(np.outer(u1, v1) + np.outer(u2, v2))))
    out.append(("rank 2, diagonal", from_h(np.diag([3.0, 2.0, 0.0]))))
    out.append(("rank 2, three points", moments(rng.normal(size=(3, 3)).astype(np.float32), rng.normal(size=(3, 3)).astype(np.float32))))
    out.append(("rank 1", from_h(np.outer(u1, v1))))
    out.append(("rank 1, diagonal", from_h(np.diag([5.0, 0.0, 0.0]))))
    out.append(("rank 1, second axis", from_h(np.diag([0.0, 5.0, 0.0]))))
    out.append(("rank 1, two points", moments(rng.normal(size=(2, 3)).astype(np.float32), rng.normal(size=(2, 3)).astype(np.float32))))
    out.append(("H == 0", from_h(np.zeros((3, 3)))))
    # det < 0
    Q = rot(0.3, -0.2, 0.5)
    out.append(("reflection", from_h(Q @ np.diag([3.0, 2.0, -1.0]) @ rot(-0.1, 0.4, 0.2).T)))
    out.append(("reflection, diagonal", from_h(np.diag([1.0, 1.0, -1.0]))))
    pts = (rng.normal(size=(500, 3)) * [30.0, 20.0, 1.0]).astype(np.float32)
    out.append(("mirrored cloud", moments(pts, pts * np.array([1.0, 1.0, -1.0], np.float32) @ rot(0.01, 0.02, -0.03).T.astype(np.float32))))
    # M = 0 and M = 1
    out.append(("M = 0", np.zeros(16)))
    out.append(("M = 0, sums set", from_h(np.diag([3.0, 2.0, 1.0]), 0.0)))
    out.append(("M = 1", moments(pts[:1], pts[1:2])))
    # scales, and a pair far from the origin
    R = rot(0.004, -0.003, 0.01)
    for scale in (1e-3, 1.0, 1e6):
        ps = (pts.astype(np.float64) * scale).astype(np.float32)
        qs = (ps.astype(np.float64) @ R.T + scale * np.array([0.3, -0.2, 0.05]) + rng.normal(size=ps.shape) * 0.01 * scale).astype(np.float32)
        out.append((f"scene x {scale:g}", moments(ps, qs)))
    far = np.array([1000.0, -1000.0, 40.0])
    pf = (pts.astype(np.float64) + far).astype(np.float32)
    qf = ((pts.astype(np.float64) @ R.T) + far + np.array([0.3, -0.2, 0.05]) + rng.normal(size=pts.shape) * 0.01).astype(np.float32)
    out.append(("1 000 m from the origin", moments(pf, qf)))
    return out


def seeded(n, seed=7):
    """(n, 16): moments of small random clouds and their moved copies — extents, scales (1e-3 .. 1e6), rotations (0.0025 deg .. anything), noise, offsets
    and counts drawn per case; one case in sixteen mirrored; counts 1, 2 and 3 (rank-deficient H) among them"""
    rng = np.random.default_rng(seed)
    K = 8
    cnt = rng.integers(1, K + 1, size=n)
    scale = 10.0 ** rng.uniform(-3.0, 6.0, size=n)
    ext = np.stack([rng.uniform(0.5, 30.0, n), rng.uniform(0.5, 20.0, n), rng.uniform(0.01, 2.0, n)], 1)
    ang = np.deg2rad(10.0 ** rng.uniform(np.log10(0.0025), np.log10(180.0), size=(n, 3))) * rng.choice([-1.0, 1.0], size=(n, 3))
    off = rng.normal(size=(n, 3)) * rng.choice([0.0, 1.0, 1000.0], size=(n, 1))
    noise = rng.choice([0.0, 0.01, 0.3], size=n)
    mirror = rng.integers(0, 16, size=n) == 0
    sums = np.empty((n, 16))
    for i in range(n):
        p = ((rng.normal(size=(cnt[i], 3)) * ext[i] + off[i]) * scale[i]).astype(np.float32)
        R = rot(*ang[i])
        if mirror[i]:
            R = R @ np.diag([1.0, 1.0, -1.0])
        q = (p.astype(np.float64) @ R.T + scale[i] * (rng.normal(size=3) * 0.2) + rng.normal(size=p.shape) * noise[i] * scale[i]).astype(np.float32)
        sums[i] = moments(p, q)
    return sums
