"""CPU: global motion from tracks -- drivers.motion_table_torch / motion_fit_torch (the consensus similarity rule of pips_motion_fit,
include/pips_hip.h), MotionEstimator(engine="torch") and motion_path.  The rule is restated here as a plain-Python loop over pairs,
hypotheses and points on Python ints (which cannot overflow) and Python floats (IEEE doubles, an operation a rounding).  (The
kernels and ``engine="library"``: tests/test_motion_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
NAN, INF = float("nan"), float("inf")
VIS_LOGIT = 0.5                                                          # exactly an fp32: "vis exactly at the threshold" is not above it


def _mix(seed, g, k):
    u = (seed + 0x9E3779B9 * (g + 1) + 0x85EBCA6B * (k + 1)) & M32
    u ^= u >> 16
    u = (u * 0x85EBCA6B) & M32
    u ^= u >> 13
    u = (u * 0xC2B2AE35) & M32
    return u ^ (u >> 16)


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def _rule(trajs, vis, frame0, vis_logit, K, thr4, seed):
    """the rule, pair by pair, hypothesis by hypothesis, point by point -> (head, sums, model, flags) as nested lists"""
    t = trajs.to(torch.float32).numpy()
    v = None if vis is None else vis.to(torch.float32).numpy()
    F, n = t.shape[:2]

    def point(f, k):                                                     # the quantised point of row f, or None
        with np.errstate(over="ignore"):                                 # (3e38 x 4 is an infinity: not usable)
            s = t[f, k] * np.float32(4.0)
        if not (np.isfinite(s).all() and abs(float(s[0])) <= 8191 and abs(float(s[1])) <= 8191):
            return None
        if v is not None and not v[f, k] > np.float32(vis_logit):
            return None
        return (int(np.rint(s[0])), int(np.rint(s[1])))

    heads, sums, models, flags = [], [], [], []
    for f in range(1, F):
        rows = [(point(f - 1, k), point(f, k)) for k in range(n)]
        cols = [k for k in range(n) if rows[k][0] is not None and rows[k][1] is not None]
        m, g = len(cols), frame0 + f
        P, Q = [rows[k][0] for k in cols], [rows[k][1] for k in cols]
        best, h_best, best_in = 0, -1, []
        for h in range(K if m >= 2 else 0):
            i = (_mix(seed, g, 2 * h) * m) >> 32
            j = (_mix(seed, g, 2 * h + 1) * (m - 1)) >> 32
            j += j >= i
            d, e = _sub(P[j], P[i]), _sub(Q[j], Q[i])
            inl = []
            if d != (0, 0):
                for k in range(m):
                    r = _sub(_cmul(e, _sub(P[k], P[i])), _cmul(d, _sub(Q[k], Q[i])))
                    assert abs(r[0]) < 2 ** 31 and abs(r[1]) < 2 ** 31
                    if r[0] * r[0] + r[1] * r[1] <= thr4 * thr4 * (d[0] * d[0] + d[1] * d[1]):
                        inl.append(k)
            if len(inl) > best:
                best, h_best, best_in = len(inl), h, inl
        if best < 2:
            best, h_best, best_in = 0, -1, []
        fl = [0] * n
        for k in cols:
            fl[k] = 1
        for k in best_in:
            fl[cols[k]] = 2
        p, q = [P[k] for k in best_in], [Q[k] for k in best_in]
        S = [len(p), sum(a[0] for a in p), sum(a[1] for a in p), sum(a[0] for a in q), sum(a[1] for a in q),
             sum(a[0] * a[0] + a[1] * a[1] for a in p), sum(a[0] * b[0] + a[1] * b[1] for a, b in zip(p, q)),
             sum(a[0] * b[1] - a[1] * b[0] for a, b in zip(p, q))]
        model = [1.0, 0.0, 0.0, 0.0]
        if h_best >= 0:
            D = S[0] * S[5] - (S[1] * S[1] + S[2] * S[2])
            A = S[0] * S[6] - (S[1] * S[3] + S[2] * S[4])
            B = S[0] * S[7] - (S[1] * S[4] - S[2] * S[3])
            assert 0 < D < 2 ** 61 and abs(A) < 2 ** 61 and abs(B) < 2 ** 61
            are, aim = float(A) / float(D), float(B) / float(D)
            spx, spy, sqx, sqy, n4 = float(S[1]), float(S[2]), float(S[3]), float(S[4]), float(4 * S[0])
            model = [are, aim, (sqx - (are * spx - aim * spy)) / n4, (sqy - (aim * spx + are * spy)) / n4]
        heads.append([m, best, h_best, 0]), sums.append(S), models.append(model), flags.append(fl)
    return heads, sums, models, flags


def _f64_bits(x):
    return torch.as_tensor(x, dtype=torch.float64).reshape(-1).view(torch.int64).tolist()


def _assert_rule(trajs, vis, frame0, K, thr4, seed, vis_logit=VIS_LOGIT):
    head, sums, model, flags = drivers.motion_table_torch(trajs, vis, frame0, vis_logit, K, thr4, seed)
    P, n = max(trajs.shape[0] - 1, 0), trajs.shape[1]
    assert tuple(head.shape) == (P, 4) and tuple(sums.shape) == (P, 8) and tuple(model.shape) == (P, 4) and tuple(flags.shape) == (P, n)
    assert head.dtype == torch.int64 and sums.dtype == torch.int64 and model.dtype == torch.float64 and flags.dtype == torch.uint8
    ref = _rule(trajs, vis, frame0, vis_logit, K, thr4, seed)
    assert head.tolist() == ref[0] and sums.tolist() == ref[1] and flags.tolist() == ref[3]
    assert _f64_bits(model) == _f64_bits(ref[2] if P else [])
    return head, sums, model, flags


def _scene(F, n, seed, outliers=0.3, noise=0.25, size=(640.0, 480.0)):
    """F rows of n points: row f is row f - 1 under a similarity of its own (a rotation of up to 3 degrees, a scale within 3 %, a
    shift of up to 12 px) plus uniform noise, except that `outliers` of the columns go their own way -> trajs (F,n,2) float32"""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.rand(n, 2, generator=g, dtype=torch.float64) * torch.tensor(size, dtype=torch.float64)]
    wild = torch.rand(n, generator=g) < outliers
    for _ in range(1, F):
        ang, sc = (torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([math.radians(6.0), 0.06], dtype=torch.float64)
        a = (1.0 + float(sc)) * complex(math.cos(float(ang)), math.sin(float(ang)))
        t = (torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * 24.0
        p = rows[-1]
        q = torch.stack([a.real * p[:, 0] - a.imag * p[:, 1], a.imag * p[:, 0] + a.real * p[:, 1]], dim=1) + t
        q = q + (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * 2.0 * noise
        q[wild] += (torch.rand(int(wild.sum()), 2, generator=g, dtype=torch.float64) - 0.5) * 120.0
        rows.append(q)
    return torch.stack(rows).to(torch.float32)


# ---------------------------------------------------------------------------------------------- the rule
def test_mix_gives_the_hand_computed_words():
    """mix(k) of frame g worked out by hand (Python ints, the header's line), against the tensor form of the torch twin"""
    words = {(0, 0, 0): 0x024CDEBC, (1234, 7, 5): 0x05610854, (M32, 2 ** 31 - 2, 2047): 0xF7C832F7, (1, 0, 1): 0x082B2728}
    for (seed, g, k), w in words.items():
        assert _mix(seed, g, k) == w, (seed, g, k, hex(_mix(seed, g, k)))
        assert int(drivers.motion_mix(seed, g, k)) == w
    k = torch.arange(0, 2048)
    got = drivers.motion_mix(1234, 7, k)
    assert got.dtype == torch.int64 and got.tolist() == [_mix(1234, 7, i) for i in range(2048)]
    assert drivers.motion_mix(M32, 2 ** 31 - 2, k).tolist() == [_mix(M32, 2 ** 31 - 2, i) for i in range(2048)]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 65])
def test_torch_form_is_the_rule_restated(n):
    """F = 1 / 2 / 5 and K = 1 / 64 / 257 on scenes with noise and outliers, with and without vis, frame0 = 0 and > 0"""
    for F in (1, 2, 5):
        trajs = _scene(F, n, 100 * F + n)
        g = torch.Generator().manual_seed(n)
        vis = torch.randn(F, n, generator=g) + 1.0
        for K, frame0, v in ((1, 0, None), (64, 0, vis), (257, 31, None), (64, 2 ** 31 - 1 - F, vis)):
            head, _, _, flags = _assert_rule(trajs, v, frame0, K, 8, 1234)
            if F > 1 and n == 65 and K >= 64 and v is None:
                assert int(head[:, 1].min()) >= 30 and int((flags == 1).sum()) > 0           # a consensus, and tracks outside it


def test_the_named_columns_are_judged_as_the_rule_says():
    """NaN, +-inf, |x| = 2047.75 (usable) and 2048.0 (not), in either row and either component; vis at, above and below the threshold
    and NaN; halves that round to even"""
    base = _scene(2, 24, 5, outliers=0.0, noise=0.0)
    t = base.clone()
    t[0, 0, 0], t[1, 1, 1], t[0, 2, 0], t[1, 3, 1] = NAN, NAN, INF, -INF
    t[0, 4], t[1, 4] = torch.tensor([2047.75, -2047.75]), torch.tensor([-2047.75, 2047.75])
    t[0, 5, 0], t[1, 6, 1], t[0, 7, 0] = 2048.0, -2048.0, 3.0e38
    t[0, 8], t[1, 8] = torch.tensor([10.125, 10.375]), torch.tensor([-10.125, -10.375])       # 40.5 -> 40, 41.5 -> 42
    head, _, _, flags = _assert_rule(t, None, 0, 64, 8, 7)
    assert flags[0, :8].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and int(head[0, 0]) == 24 - 7
    vis = torch.full((2, 24), 3.0)
    vis[0, 9], vis[1, 10], vis[0, 11], vis[1, 12] = VIS_LOGIT, VIS_LOGIT, NAN, -1.0
    vis[0, 13] = float(np.nextafter(np.float32(VIS_LOGIT), np.float32(1.0)))
    head, _, _, flags = _assert_rule(t, vis, 0, 64, 8, 7)
    assert flags[0, 9:13].tolist() == [0, 0, 0, 0] and int(flags[0, 13]) >= 1 and int(head[0, 0]) == 24 - 11


def test_pairs_without_a_model_and_the_smallest_ones():
    nan = torch.full((3, 9, 2), NAN)
    head, sums, model, flags = _assert_rule(nan, None, 0, 64, 8, 1)                            # every column invalid
    assert head.tolist() == [[0, 0, -1, 0]] * 2 and model.tolist() == [[1.0, 0.0, 0.0, 0.0]] * 2 and int(flags.sum()) == 0
    two = nan.clone()
    two[:, 2], two[:, 7] = torch.tensor([5.0, 6.0]), torch.tensor([50.0, 9.0])
    two[1:, 7] += torch.tensor([1.0, 2.0])
    head, sums, model, flags = _assert_rule(two, None, 3, 5, 4, 1)                             # m == 2: both are the consensus
    assert head[:, :2].tolist() == [[2, 2], [2, 2]] and flags[0].tolist() == [0, 0, 2, 0, 0, 0, 0, 2, 0]
    same = torch.full((2, 9, 2), 33.25)
    same[1] = 40.0
    head, sums, model, flags = _assert_rule(same, None, 0, 64, 8, 1)                           # every hypothesis has d = 0
    assert head.tolist() == [[9, 0, -1, 0]] and flags.tolist() == [[1] * 9] and int(sums.abs().sum()) == 0
    assert model.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    one = nan[:2].clone()
    one[:, 4] = 1.0
    assert _assert_rule(one, None, 0, 64, 8, 1)[0].tolist() == [[1, 0, -1, 0]]                 # m == 1


def test_ties_go_to_the_lowest_hypothesis_and_the_widest_products_fit():
    g = torch.Generator().manual_seed(3)
    p = torch.randint(-400, 400, (40, 2), generator=g).float() * 0.25
    t = torch.stack([p, p + torch.tensor([3.25, -1.5])])
    head, _, model, _ = _assert_rule(t, None, 0, 257, 4, 9)                                    # pure translation: most hypotheses tie
    i, j = (_mix(9, 1, 0) * 40) >> 32, (_mix(9, 1, 1) * 39) >> 32
    j += j >= i
    assert not torch.equal(p[i], p[j]) and head.tolist() == [[40, 40, 0, 0]] and model.tolist() == [[1.0, 0.0, 3.25, -1.5]]
    c = 2047.75
    corners = torch.tensor([[c, c], [-c, c], [-c, -c], [c, -c]])
    t = torch.stack([corners, corners[[2, 3, 0, 1]], -corners[[1, 2, 3, 0]]])                  # a half turn, then a quarter turn
    for thr4 in (1, 1024):
        head, sums, model, _ = _assert_rule(t, None, 5, 64, thr4, 2)
        assert head[:, :2].tolist() == [[4, 4], [4, 4]] and model[0].tolist() == [-1.0, 0.0, 0.0, 0.0]
        assert int(sums[0, 5]) == 8 * 8191 * 8191
    far = torch.cat([corners, torch.tensor([[c, -c + 300.0], [0.25, 0.0]])])                   # thr4 = 1024 between the far corners
    _assert_rule(torch.stack([far, far[[2, 3, 0, 1, 5, 4]]]), None, 0, 64, 1024, 2)


def test_bad_arguments_are_rejected():
    t = torch.zeros(3, 4, 2)
    for bad in (dict(K=0), dict(K=1025), dict(thr4=0), dict(thr4=1025), dict(frame0=-1), dict(frame0=2 ** 31 - 3), dict(seed=-1),
                dict(seed=2 ** 32)):
        a = dict(dict(frame0=0, K=8, thr4=8, seed=0), **bad)
        with pytest.raises(ValueError):
            drivers.motion_table_torch(t, None, a["frame0"], 0.0, a["K"], a["thr4"], a["seed"])
    for shape in ((3, 4), (3, 4, 3)):
        with pytest.raises(ValueError):
            drivers.motion_table_torch(torch.zeros(shape), None, 0, 0.0, 8, 8, 0)
    with pytest.raises(ValueError):
        drivers.motion_table_torch(t, torch.zeros(3, 5), 0, 0.0, 8, 8, 0)
    with pytest.raises(ValueError):
        drivers.motion_table_torch(torch.zeros(2, 65537, 2), None, 0, 0.0, 8, 8, 0)
    t4 = t.unsqueeze(0)
    for bad in (dict(thr=0.3), dict(thr=0.0), dict(thr=256.25), dict(thr=True), dict(thr="2"), dict(hypotheses=0), dict(hypotheses=1025),
                dict(hypotheses=2.5), dict(vis_thr=0.0), dict(vis_thr=1.0), dict(seed=-1), dict(frame0=-1), dict(ids=[0, 1, 2]),
                dict(ids=[0, 1, 2, 2])):
        with pytest.raises(ValueError):
            drivers.motion_fit_torch(t4, **bad)
        if "ids" not in bad and "frame0" not in bad:
            with pytest.raises(ValueError):
                drivers.MotionEstimator(engine="torch", **bad)
    with pytest.raises(ValueError):
        drivers.motion_fit_torch(t)
    with pytest.raises(ValueError):
        drivers.motion_fit_torch(t4, vis=torch.zeros(1, 3, 5))
    with pytest.raises(ValueError):
        drivers.MotionEstimator(engine="cpu")
    with pytest.raises(ValueError):
        drivers.MotionEstimator(engine="torch", trail=3)
    assert drivers.motion_fit_torch(t4, thr=0.25)[0].shape == (2, 4) and drivers.motion_fit_torch(t4, thr=256)[0].shape == (2, 4)


# ---------------------------------------------------------------------------------------------- the driver
def test_driver_returns_the_tables_and_ids_sort_the_columns():
    trajs, g = _scene(4, 30, 8), torch.Generator().manual_seed(8)
    vis = torch.randn(4, 30, generator=g) + 1.5
    logit = float(torch.logit(torch.tensor(0.7, dtype=torch.float32)))
    head, _, model, flags = drivers.motion_table_torch(trajs, vis, 11, logit, 32, 6, 99)
    models, inliers, valid, counts = drivers.motion_fit_torch(trajs[None], vis[None], frame0=11, thr=1.5, hypotheses=32, vis_thr=0.7, seed=99)
    assert models.dtype == torch.float64 and inliers.dtype == torch.bool and valid.dtype == torch.bool
    assert _f64_bits(models) == _f64_bits(model) and torch.equal(inliers, flags == 2) and torch.equal(valid, flags >= 1)
    assert counts.tolist() == head[:, :2].tolist() and bool((inliers & ~valid).sum() == 0) and int(inliers.sum()) > 20
    # shuffled columns with their ids: the sorted call, the flags back in the caller's order
    perm = torch.randperm(30, generator=g)
    got = drivers.motion_fit_torch(trajs[None][:, :, perm], vis[None][:, :, perm], ids=perm, frame0=11, thr=1.5, hypotheses=32,
                                   vis_thr=0.7, seed=99)
    assert _f64_bits(got[0]) == _f64_bits(models) and torch.equal(got[1], inliers[:, perm]) and torch.equal(got[2], valid[:, perm])
    assert torch.equal(got[3], counts)
    wide = drivers.motion_fit_torch(trajs[None], ids=torch.arange(30) * 7 + 3, frame0=11, thr=1.5, hypotheses=32, seed=99)
    plain = drivers.motion_fit_torch(trajs[None], frame0=11, thr=1.5, hypotheses=32, seed=99)
    assert all(torch.equal(a, b) for a, b in zip(wide, plain))                                 # only the order of the ids counts


def _life_video(T, K, seed):
    """a video by identity: K columns over T frames, NaN outside each life [born, retired]; most columns span the whole video"""
    g = torch.Generator().manual_seed(seed)
    trajs = _scene(T, K, seed)
    vis = torch.randn(T, K, generator=g) + 1.5
    born = torch.where(torch.rand(K, generator=g) < 0.6, torch.zeros(K), torch.randint(0, T, (K,), generator=g).float()).long()
    last = torch.where(torch.rand(K, generator=g) < 0.6, torch.full((K,), T - 1.0), torch.randint(0, T, (K,), generator=g).float()).long()
    last = torch.maximum(last, born)
    f = torch.arange(T).view(T, 1)
    dead = (f < born.view(1, K)) | (f > last.view(1, K))
    trajs[dead], vis[dead] = NAN, NAN
    return trajs, vis, born, last


@pytest.mark.parametrize("with_vis", [False, True])
@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_estimator_push_by_push_is_the_whole_video_call(chunk, with_vis):
    """T = 19, 40 identities that are born and retired on the way; a push holds the identities alive in it, in a shuffled order
    of their own: the models, inliers, valid and counts of every pair equal those of one call on the video by identity"""
    T, K = 19, 40
    trajs, vis, born, last = _life_video(T, K, 21)
    kw = dict(thr=1.5, hypotheses=48, vis_thr=0.6, seed=5)
    whole = drivers.motion_fit_torch(trajs[None], vis[None] if with_vis else None, ids=torch.arange(K), **kw)
    assert int(whole[3][:, 1].min()) >= 8 and len(set(whole[3][:, 0].tolist())) > 3            # consensus, and columns come and go
    est = drivers.MotionEstimator(engine="torch", **kw)
    g = torch.Generator().manual_seed(22)
    got, pair = [], 0
    assert est.step(0, trajs[None][:, :0, :0]).shape == (0, 4)                                 # a push without rows
    for f0 in range(0, T, chunk):
        f1 = min(f0 + chunk, T)
        alive = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
        ids = alive[torch.randperm(alive.numel(), generator=g)]
        models = est.step(f0, trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids] if with_vis else None, ids=ids)
        P = f1 - f0 - (1 if f0 == 0 else 0)
        assert tuple(models.shape) == (P, 4) and tuple(est.inliers.shape) == (P, ids.numel()) and est.T == f1
        assert torch.equal(est.inliers, whole[1][pair:pair + P][:, ids]) and torch.equal(est.valid, whole[2][pair:pair + P][:, ids])
        assert torch.equal(est.counts, whole[3][pair:pair + P])
        assert int(whole[1][pair:pair + P].sum()) == int(est.inliers.sum())                    # nobody outside the push is an inlier
        got.append(models)
        pair += P
    assert pair == T - 1 and _f64_bits(torch.cat(got)) == _f64_bits(whole[0])
    with pytest.raises(ValueError):
        est.step(T + 1, trajs[None][:, :1])                                                    # a gap
    with pytest.raises(ValueError):
        est.step(T, trajs[None][:, :1, :5], ids=[0, 1, 2, 3])
    with pytest.raises(ValueError):
        est.step(T, trajs[None][:, :1], None if with_vis else vis[None][:, :1])                # vis on every step or on none


def test_estimator_with_stable_columns_needs_no_ids():
    trajs = _scene(9, 25, 31)
    whole = drivers.motion_fit_torch(trajs[None], hypotheses=32, seed=3)
    est = drivers.MotionEstimator(engine="torch", hypotheses=32, seed=3)
    got = torch.cat([est.step(f0, trajs[None][:, f0:f0 + 4]) for f0 in range(0, 9, 4)])
    assert _f64_bits(got) == _f64_bits(whole[0])
    with pytest.raises(ValueError):
        est.step(9, trajs[None][:, :1, :20])                                                   # the columns changed without ids


def test_motion_path_is_the_matrix_product_inverted():
    g = torch.Generator().manual_seed(4)
    P = 12
    ang, sc = (torch.rand(P, generator=g, dtype=torch.float64) - 0.5) * 0.2, 1.0 + (torch.rand(P, generator=g, dtype=torch.float64) - 0.5) * 0.1
    models = torch.stack([sc * torch.cos(ang), sc * torch.sin(ang), torch.randn(P, generator=g, dtype=torch.float64) * 9.0,
                          torch.randn(P, generator=g, dtype=torch.float64) * 9.0], dim=1)
    path = drivers.motion_path(models)
    assert tuple(path.shape) == (P + 1, 4) and path.dtype == torch.float64 and path[0].tolist() == [1.0, 0.0, 0.0, 0.0]

    def mat(r):
        return torch.tensor([[r[0], -r[1], r[2]], [r[1], r[0], r[3]], [0.0, 0.0, 1.0]], dtype=torch.float64)

    M = torch.eye(3, dtype=torch.float64)
    for f in range(P):
        M = mat(models[f].tolist()) @ M                                                        # frame 0 -> frame f + 1
        assert torch.allclose(mat(path[f + 1].tolist()) @ M, torch.eye(3, dtype=torch.float64), rtol=0.0, atol=1e-9)
    assert drivers.motion_path(torch.zeros(0, 4)).tolist() == [[1.0, 0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        drivers.motion_path(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        drivers.motion_path(torch.zeros(1, 4))


# ---------------------------------------------------------------------------------------------- what the fit means
def test_an_exact_translation_is_recovered_exactly():
    """60 points on the quarter-pixel grid moved by (5.25, -3.75) px, 30 % of them instead put at least 8 px from where the shift
    would put them; thr = 1.0.  The conditions are asserted first: the grid, the distance of the outliers, and that a hypothesis of
    the 64 draws two different planted points.  Then the inliers are the planted set, a = 1 + 0i and t the shift, all exact."""
    n, K, seed, shift = 60, 64, 11, torch.tensor([5.25, -3.75])
    g = torch.Generator().manual_seed(0)
    p = torch.randint(0, 4 * 600, (n, 2), generator=g).float() * 0.25
    wild = torch.zeros(n, dtype=torch.bool)
    wild[torch.randperm(n, generator=g)[:18]] = True
    off = torch.randint(8 * 4, 60 * 4, (n, 2), generator=g).float() * 0.25 * (torch.randint(0, 2, (n, 2), generator=g).float() * 2 - 1)
    q = p + shift + off * wild.view(n, 1)
    assert torch.equal(p * 4, (p * 4).round()) and torch.equal(q * 4, (q * 4).round()) and float(q.abs().max()) < 2047
    assert float((q - p - shift)[wild].norm(dim=1).min()) >= 8.0 and bool(((q - p - shift)[~wild] == 0).all()) and int(wild.sum()) == 18
    planted = []
    for h in range(K):
        i, j = (_mix(seed, 7, 2 * h) * n) >> 32, (_mix(seed, 7, 2 * h + 1) * (n - 1)) >> 32
        j += j >= i
        if not wild[i] and not wild[j] and not torch.equal(p[i], p[j]):
            planted.append(h)
    assert planted
    models, inliers, valid, counts = drivers.motion_fit_torch(torch.stack([p, q])[None], frame0=6, thr=1.0, hypotheses=K, seed=seed)
    assert bool(valid.all()) and torch.equal(inliers[0], ~wild) and counts.tolist() == [[60, 42]]
    assert models.tolist() == [[1.0, 0.0, 5.25, -3.75]]


MAX_ERR = 0.72


@pytest.mark.parametrize("n,K", [(40, 64), (257, 64), (2048, 256)])
def test_a_noisy_similarity_is_recovered_within_its_error_bound(n, K):
    """Rotation 2 degrees, scale 1.02, shift (7.3, -4.1) px, +-0.25 px uniform noise on q, 30 % outliers thrown 8..100 px from their
    place; thr = 2.0, torch seed 0, hash seed 1234, the pair that ends on frame 7.  First the condition, with the torch form alone:
    the inliers are the planted set, no misses and no false inliers (deterministic for the seeds).  Then the error, which the fit
    on exactly the planted set cannot exceed: with the quantised p as the regressor, q = a p + t + err with |err| <= sqrt(2) (0.125
    |a| + 0.25 + 0.125) = 0.7106 px a point (the quantisation of p and q to quarter pixels and the noise; 0.72 with the fp32
    rounding of the inputs).  A least-squares similarity averages: at the centroid of the planted points it is off by at most
    max |err|, and |a - a_true| <= max |err| sqrt(N / S|p - c|^2) = max |err| / rms radius (Cauchy-Schwarz)."""
    g = torch.Generator().manual_seed(0)
    a = 1.02 * complex(math.cos(math.radians(2.0)), math.sin(math.radians(2.0)))
    t = torch.tensor([7.3, -4.1], dtype=torch.float64)
    p = (torch.rand(n, 2, generator=g, dtype=torch.float64) * torch.tensor([640.0, 480.0], dtype=torch.float64)).float().double()
    wild = torch.zeros(n, dtype=torch.bool)
    wild[torch.randperm(n, generator=g)[:(3 * n) // 10]] = True
    true_q = torch.stack([a.real * p[:, 0] - a.imag * p[:, 1], a.imag * p[:, 0] + a.real * p[:, 1]], dim=1) + t
    q = true_q + (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * 0.5
    r, phi = 8.0 + torch.rand(n, generator=g, dtype=torch.float64) * 92.0, torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    q[wild] = (true_q + torch.stack([r * torch.cos(phi), r * torch.sin(phi)], dim=1))[wild]
    trajs = torch.stack([p, q]).float()[None]
    assert float((trajs[0, 1].double() - true_q)[wild].norm(dim=1).min()) >= 7.99 and float(trajs.abs().max()) < 2047
    models, inliers, valid, counts = drivers.motion_fit_torch(trajs, frame0=6, thr=2.0, hypotheses=K, seed=1234)
    missed, false_in = int((~inliers[0] & ~wild).sum()), int((inliers[0] & wild).sum())
    print(f"n={n} K={K}: {int(inliers.sum())} inliers of {int((~wild).sum())} planted, {missed} missed, {false_in} false")
    assert bool(valid.all()) and missed == 0 and false_in == 0                                 # the condition
    pin = p[~wild]
    c = pin.mean(dim=0)
    rms = float(((pin - c) ** 2).sum(dim=1).mean().sqrt())
    got_a, got_t = complex(float(models[0, 0]), float(models[0, 1])), complex(float(models[0, 2]), float(models[0, 3]))
    at_c = got_a * complex(float(c[0]), float(c[1])) + got_t - (a * complex(float(c[0]), float(c[1])) + complex(float(t[0]), float(t[1])))
    print(f"n={n} K={K}: |a - a_true| = {abs(got_a - a):.3e} (bound {MAX_ERR / rms:.3e}), at the centroid {abs(at_c):.3e} px (bound {MAX_ERR})")
    assert abs(got_a - a) <= MAX_ERR / rms and abs(at_c) <= MAX_ERR


# ---------------------------------------------------------------------------------------------- the ABI
def test_motion_fit_is_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_motion_fit" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)      # the history comment
    for words in ("0x9E3779B9", "0x85EBCA6B", "0xC2B2AE35", "j += (j >= i)", "round-half-even", "|r|^2 <= thr4^2 |d|^2",
                  "ties go to the lowest h", "never fused"):
        assert words in hdr, words                                         # the rule stands in the header
    for name, value in (("QUARTER_MAX", ops.MOTION_QUARTER_MAX), ("HYPS_MAX", ops.MOTION_HYPS_MAX), ("THR4_MAX", ops.MOTION_THR4_MAX),
                        ("N_MAX", ops.MOTION_N_MAX)):
        assert int(re.search(rf"#define PIPS_MOTION_{name}\s+(\d+)", hdr).group(1)) == value
    common = open(os.path.join(ROOT, "pips_amd", "csrc", "common.h")).read()
    assert int(re.search(r"constexpr int MOTION_TILE = (\d+);", common).group(1)) == ops.MOTION_TILE
    assert int(re.search(r"constexpr int MOTION_HYPS = (\d+);", common).group(1)) == ops.MOTION_HYPS
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_motion_fit\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 16
    proto = re.search(r"\bsize_t\s+pips_motion_workspace_bytes\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 3
    res, args = _lib.SIGNATURES["pips_motion_fit"]
    assert res is ctypes.c_int and len(args) == 16 and args[5] is ctypes.c_float and args[8] is ctypes.c_int
    assert args[14] is ctypes.c_size_t
    assert _lib.SIGNATURES["pips_motion_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert "motion.hip" in _build.SOURCES and any(h.endswith("fp_rn.h") for h in _build.headers())
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_motion_fit") and hasattr(raw, "pips_motion_workspace_bytes") and callable(ops.motion_fit)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the sizing query is a host function: per pair 8 bytes a column, the count and a key per block of 64 hypotheses
    size = lib.pips_motion_workspace_bytes
    assert size(5, 100, 256) == 4 * (800 + 4 * 5) and size(2, 1, 1) == 8 + 8 and size(2, 65536, 1024) == 8 * 65536 + 4 * 17
    assert size(3, 7, 64) == 2 * (56 + 8) and size(3, 7, 65) == 2 * (56 + 12) and ops.motion_workspace_bytes(3, 7, 65) == 136
    assert size(1, 100, 64) == 0 and size(0, 100, 64) == 0 and size(5, 0, 64) == 0
    assert size(-1, 8, 8) == 0 and size(5, -1, 8) == 0 and size(5, 65537, 8) == 0 and size(5, 8, 0) == 0 and size(5, 8, 1025) == 0
    assert size((1 << 24) + 1, 8, 8) == 0 and size(1 << 24, 8, 8) > 0
    # the host-side rejections need no device: nothing is launched

    def call(F=3, n=8, frame0=0, logit=0.0, K=8, thr4=8):
        return lib.pips_motion_fit(None, None, F, n, frame0, logit, K, thr4, 0, None, None, None, None, None, 0, None)

    for bad in (dict(F=-1), dict(F=(1 << 24) + 1), dict(n=-1), dict(n=65537), dict(K=0), dict(K=1025), dict(thr4=0), dict(thr4=1025),
                dict(frame0=-1), dict(frame0=2 ** 31 - 3), dict(logit=NAN), dict()):
        assert call(**bad) == -1, bad
        assert lib.pips_last_error().decode().startswith("motion_fit:"), bad
    assert call(F=0) == 0 and call(F=1) == 0 and call(F=1, n=0) == 0                           # nothing to fit, nothing launched
