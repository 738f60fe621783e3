"""CPU: moving objects from tracks -- drivers.motion_layers_table_torch / motion_layers_torch (the motion-layer rule of
pips_motion_layers, include/pips_hip.h), link_layers and MotionLayers(engine="torch").  The rule is restated here as a plain-Python
loop over pairs, layers, hypotheses and points on Python ints and floats, in the style of tests/test_motion.py's ``_rule``.  (The
kernels and ``engine="library"``: tests/test_motion_layers_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers, ops
from test_motion import M32, NAN, VIS_LOGIT, _cmul, _f64_bits, _life_video, _mix, _scene, _sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_SEED = 0x632BE5AB


def _layers_rule(trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev_layer=None):
    """the rule, pair by pair, layer by layer, hypothesis by hypothesis, point by point -> (head [P][L][4], sums [P][L][8], model
    [P][L][4], box [P][L][4], layer [P][n], overlap [P][L][L]) as nested lists"""
    t = trajs.to(torch.float32).numpy()
    v = None if vis is None else vis.to(torch.float32).numpy()
    F, n = t.shape[:2]

    def point(f, k):                                                     # the quantised point of row f, or None
        with np.errstate(over="ignore"):
            s = t[f, k] * np.float32(4.0)
        if not (np.isfinite(s).all() and abs(float(s[0])) <= 8191 and abs(float(s[1])) <= 8191):
            return None
        if v is not None and not v[f, k] > np.float32(vis_logit):
            return None
        return (int(np.rint(s[0])), int(np.rint(s[1])))

    heads, sums, models, boxes, layers, overlaps = [], [], [], [], [], []
    before = None if prev_layer is None else [int(x) for x in prev_layer.tolist()]
    for f in range(1, F):
        rows = [(point(f - 1, k), point(f, k)) for k in range(n)]
        cols = [k for k in range(n) if rows[k][0] is not None and rows[k][1] is not None]
        label = [255] * n
        for k in cols:
            label[k] = 254
        g = frame0 + f
        hd, sm, md, bx = [], [], [], []
        for l in range(L):
            m, seed_l = len(cols), (seed + l * LAYER_SEED) & M32
            P, Q = [rows[k][0] for k in cols], [rows[k][1] for k in cols]
            best, h_best, best_in = 0, -1, []
            for h in range(K if m >= 2 else 0):
                i = (_mix(seed_l, g, 2 * h) * m) >> 32
                j = (_mix(seed_l, g, 2 * h + 1) * (m - 1)) >> 32
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
            if best < (2 if l == 0 else min_in):
                best, h_best, best_in = 0, -1, []
            p, q = [P[k] for k in best_in], [Q[k] for k in best_in]
            S = [len(p), sum(a[0] for a in p), sum(a[1] for a in p), sum(a[0] for a in q), sum(a[1] for a in q),
                 sum(a[0] * a[0] + a[1] * a[1] for a in p), sum(a[0] * b[0] + a[1] * b[1] for a, b in zip(p, q)),
                 sum(a[0] * b[1] - a[1] * b[0] for a, b in zip(p, q))]
            model, box = [1.0, 0.0, 0.0, 0.0], [0, 0, 0, 0]
            if h_best >= 0:
                D = S[0] * S[5] - (S[1] * S[1] + S[2] * S[2])
                A = S[0] * S[6] - (S[1] * S[3] + S[2] * S[4])
                B = S[0] * S[7] - (S[1] * S[4] - S[2] * S[3])
                assert 0 < D < 2 ** 61 and abs(A) < 2 ** 61 and abs(B) < 2 ** 61
                are, aim = float(A) / float(D), float(B) / float(D)
                spx, spy, sqx, sqy, n4 = float(S[1]), float(S[2]), float(S[3]), float(S[4]), float(4 * S[0])
                model = [are, aim, (sqx - (are * spx - aim * spy)) / n4, (sqy - (aim * spx + are * spy)) / n4]
                box = [min(a[0] for a in q), min(a[1] for a in q), max(a[0] for a in q), max(a[1] for a in q)]
            for k in best_in:
                label[cols[k]] = l
            gone = set(best_in)
            cols = [c for k, c in enumerate(cols) if k not in gone]                            # the inliers leave, the order stays
            hd.append([m, best, h_best, 0]), sm.append(S), md.append(model), bx.append(box)
        over = [[0] * L for _ in range(L)]
        if before is not None:
            for k in range(n):
                if label[k] < L and before[k] < L:
                    over[label[k]][before[k]] += 1
        heads.append(hd), sums.append(sm), models.append(md), boxes.append(bx), layers.append(label), overlaps.append(over)
        before = label
    return heads, sums, models, boxes, layers, overlaps


def _assert_layers(trajs, vis, frame0, K, thr4, seed, L, min_in, prev_layer=None, vis_logit=VIS_LOGIT):
    got = drivers.motion_layers_table_torch(trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev_layer)
    head, sums, model, box, layer, overlap = got
    P, n = max(trajs.shape[0] - 1, 0), trajs.shape[1]
    assert tuple(head.shape) == (P, L, 4) and tuple(sums.shape) == (P, L, 8) and tuple(model.shape) == (P, L, 4)
    assert tuple(box.shape) == (P, L, 4) and tuple(layer.shape) == (P, n) and tuple(overlap.shape) == (P, L, L)
    assert head.dtype == torch.int64 and sums.dtype == torch.int64 and model.dtype == torch.float64 and box.dtype == torch.int64
    assert layer.dtype == torch.uint8 and overlap.dtype == torch.int64
    ref = _layers_rule(trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev_layer)
    assert head.tolist() == ref[0] and sums.tolist() == ref[1] and box.tolist() == ref[3]
    assert layer.tolist() == ref[4] and overlap.tolist() == ref[5]
    assert _f64_bits(model) == _f64_bits(ref[2] if P else [])
    return got


# ---------------------------------------------------------------------------------------------- the rule
def test_the_layer_seed_is_the_hand_computed_word():
    """seed_1 = seed + 0x632BE5AB and the word mix draws from it, worked out by hand; the wrap-around of seed_3"""
    assert drivers.MOTION_LAYER_SEED == LAYER_SEED == 0x632BE5AB
    assert (1234 + 1 * LAYER_SEED) & M32 == 0x632BEA7D and _mix(0x632BEA7D, 7, 5) == 0x65A616A6
    assert int(drivers.motion_mix(0x632BEA7D, 7, 5)) == 0x65A616A6
    assert (0xF0000000 + 3 * LAYER_SEED) & M32 == 0x1983B101
    # the twin draws layer 1's winner from that seed: twelve columns shift one way (the camera), five another and three go ways of
    # their own.  Layer 0's winner is the lowest h whose two draws are both on the camera, layer 1's the lowest h -- drawn from seed_1
    # on its list of eight -- whose two draws are both among the five: found here from the hand-checked mix alone
    g = torch.Generator().manual_seed(1)
    p = torch.randperm(2000, generator=g)[:40].view(20, 2).float() * 0.25 + 3.0                # (all different)
    shift = torch.tensor([[2.0, 1.0]] * 12 + [[-30.0, 40.5]] * 5 + [[100.0, -60.0], [137.0, -113.0], [-174.0, 166.0]])
    head = _assert_layers(torch.stack([p, p + shift]), None, 6, 32, 4, 0xF0000000, 4, 5)[0]
    assert head[0, :2, :2].tolist() == [[20, 12], [8, 5]]
    for l, seed_l, mine in ((0, 0xF0000000, 12), (1, (0xF0000000 + LAYER_SEED) & M32, 5)):
        m = int(head[0, l, 0])
        first = None
        for h in range(32):
            i, j = (_mix(seed_l, 7, 2 * h) * m) >> 32, (_mix(seed_l, 7, 2 * h + 1) * (m - 1)) >> 32
            j += j >= i
            if i < mine and j < mine:
                first = h
                break
        assert first is not None and int(head[0, l, 2]) == first, l


def test_a_layer_that_takes_nothing_by_hand():
    """four columns: three move by (1, 0), the fourth by (0, 9).  Layer 0 takes the three; layer 1's list is one column long: no
    model, nothing leaves; layer 2 sees the same list"""
    p = torch.tensor([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0], [20.0, 20.0]])
    q = p + torch.tensor([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 9.0]])
    head, sums, model, box, layer, overlap = _assert_layers(torch.stack([p, q]), None, 0, 64, 4, 3, 3, 2)
    assert head[0].tolist()[0][:2] == [4, 3] and head[0, 1].tolist() == [1, 0, -1, 0] and head[0, 2].tolist() == [1, 0, -1, 0]
    assert layer.tolist() == [[0, 0, 0, 254]] and model[0].tolist() == [[1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]]
    assert sums[0, 0].tolist() == [3, 40, 40, 52, 40, 3200, 3360, -160] and int(sums[0, 1:].abs().sum()) == 0
    assert box[0].tolist() == [[4, 0, 44, 40], [0, 0, 0, 0], [0, 0, 0, 0]] and int(overlap.sum()) == 0


@pytest.mark.parametrize("n", [0, 1, 2, 3, 24, 70])
def test_torch_form_is_the_rule_restated(n):
    """F = 1 / 2 / 5, L = 1 / 2 / 4 / 8, with and without vis, min_in small enough that the outliers of the scene form layers too,
    prev_layer given and not"""
    found = 0
    for F in (1, 2, 5):
        trajs = _scene(F, n, 100 * F + n, outliers=0.4)
        g = torch.Generator().manual_seed(n)
        vis = torch.randn(F, n, generator=g) + 1.0
        prev = torch.randint(0, 10, (n,), generator=g).to(torch.uint8)
        prev[prev == 8], prev[prev == 9] = 254, 255
        for L, K, frame0, min_in in ((1, 1, 0, 2), (2, 64, 0, 3), (4, 33, 31, 2), (8, 64, 2 ** 31 - 1 - F, 2)):
            for v in (None, vis):
                head = _assert_layers(trajs, v, frame0, K, 8, 1234, L, min_in, prev if (L + F) % 2 else None)[0]
                found += int((head[:, 1:, 2] >= 0).sum())
    assert n < 24 or found > 10                                                                # layers above 0 were found


@pytest.mark.parametrize("n,F,L", [(0, 3, 4), (1, 2, 1), (3, 1, 2), (24, 5, 4), (70, 3, 8)])
def test_layer_0_is_motion_fit(n, F, L):
    trajs = _scene(F, n, 7 + n)
    g = torch.Generator().manual_seed(n)
    for vis in (None, torch.randn(F, n, generator=g) + 1.0):
        fit = drivers.motion_table_torch(trajs, vis, 5, VIS_LOGIT, 64, 8, 99)
        head, sums, model, _, layer, _ = drivers.motion_layers_table_torch(trajs, vis, 5, VIS_LOGIT, 64, 8, 99, L, 4)
        assert torch.equal(head[:, 0], fit[0]) and torch.equal(sums[:, 0], fit[1]) and _f64_bits(model[:, 0]) == _f64_bits(fit[2])
        assert torch.equal(layer == 0, fit[3] == 2) and torch.equal(layer == 255, fit[3] == 0)


def _two_shifts(s, extra=0):
    """ten columns on the quarter grid that move by (2, 1), s that move by (-30, 40.5) and `extra` that each go a way of their own"""
    g = torch.Generator().manual_seed(s)
    n = 10 + s + extra
    p = torch.randperm(2000, generator=g)[:2 * n].view(n, 2).float() * 0.25
    shift = torch.zeros(n, 2)
    shift[:10], shift[10:10 + s] = torch.tensor([2.0, 1.0]), torch.tensor([-30.0, 40.5])
    for k in range(extra):
        shift[10 + s + k] = torch.tensor([100.0 + 37.0 * k, -60.0 - 53.0 * k])
    return torch.stack([p, p + shift])


def test_min_in_at_the_boundary_and_need_0_stays_2():
    """layer 1's best score is exactly 5 (asserted): min_in = 5 gives a model, min_in = 6 none, and then layer 2 sees layer 1's list"""
    t = _two_shifts(5, extra=2)
    head, _, model, _, layer, _ = _assert_layers(t, None, 0, 256, 4, 11, 3, 5)
    assert head[0, :, :2].tolist() == [[17, 10], [7, 5], [2, 0]] and int(head[0, 1, 2]) >= 0 and int(head[0, 2, 2]) == -1
    assert layer[0].tolist() == [0] * 10 + [1] * 5 + [254] * 2 and model[0, 1].tolist() == [1.0, 0.0, -30.0, 40.5]
    head, _, model, _, layer, _ = _assert_layers(t, None, 0, 256, 4, 11, 3, 6)
    assert head[0, :, :2].tolist() == [[17, 10], [7, 0], [7, 0]] and head[0, 1:, 2].tolist() == [-1, -1]   # m_2 == m_1: nothing left
    assert layer[0].tolist() == [0] * 10 + [254] * 7 and model[0, 1].tolist() == [1.0, 0.0, 0.0, 0.0]
    # need_0 = 2 whatever min_in: two valid columns are the camera
    two = torch.full((2, 9, 2), NAN)
    two[:, 2], two[:, 7] = torch.tensor([5.0, 6.0]), torch.tensor([50.0, 9.0])
    two[1, 7] += torch.tensor([1.0, 2.0])
    head, _, _, _, layer, _ = _assert_layers(two, None, 3, 5, 4, 1, 2, 8)
    assert head[0].tolist()[0][:2] == [2, 2] and int(head[0, 0, 2]) >= 0 and layer[0].tolist() == [255, 255, 0, 255, 255, 255, 255, 0, 255]
    assert head[0, 1].tolist() == [0, 0, -1, 0]


def test_box_and_overlap_agree_with_loops():
    """the box from the labels and the quantised row; the overlap from the labels of two pairs; prev_layer given and NULL, with 254
    and 255 (and labels >= L) counting nowhere"""
    F, n, L = 4, 70, 4
    trajs = _scene(F, n, 3, outliers=0.4)
    g = torch.Generator().manual_seed(5)
    prev = torch.randint(0, 8, (n,), generator=g).to(torch.uint8)
    prev[prev == 6], prev[prev == 7] = 254, 255                                                # 4 and 5: not below L
    for given in (None, prev):
        head, _, _, box, layer, overlap = _assert_layers(trajs, None, 0, 64, 8, 2, L, 2, given)
        quarter = (trajs * 4.0).round().long()
        assert int((head[:, 1:, 2] >= 0).sum()) >= 3 and int((layer == 254).sum()) > 0
        for f in range(F - 1):
            for l in range(L):
                at = torch.nonzero(layer[f] == l).squeeze(1)
                assert at.numel() == int(head[f, l, 1])
                want = [0, 0, 0, 0] if at.numel() == 0 else quarter[f + 1][at].min(dim=0).values.tolist() + quarter[f + 1][at].max(dim=0).values.tolist()
                assert box[f, l].tolist() == want
            before = layer[f - 1] if f else given
            want = [[0] * L for _ in range(L)]
            if before is not None:
                for k in range(n):
                    a, b = int(layer[f, k]), int(before[k])
                    if a < L and b < L:
                        want[a][b] += 1
            assert overlap[f].tolist() == want
        if given is None:
            assert int(overlap[0].sum()) == 0
        else:
            assert 0 < int(overlap[0].sum()) < int((layer[0] < L).sum())


# ---------------------------------------------------------------------------------------------- linking
def _head(rows):
    """(n_in or None) per layer and pair -> head (P,L,4)"""
    return torch.tensor([[[0, c or 0, -1 if c is None else 0, 0] for c in pair] for pair in rows])


def test_link_layers_on_hand_written_tables():
    L = 4
    head = _head([[50, 10, 8, None],            # pair 0: nothing before: the camera, objects 1 and 2, no model
                  [50, 9, None, 12],            # pair 1: layer 1 overlaps both equally -> the lowest b (1); layer 3 wants b = 1 too
                  [None, 20, 6, 5],             # pair 2: no camera; min() on either side of the inequality; a new id
                  [50, 4, 4, 4]])
    overlap = torch.zeros(4, L, L, dtype=torch.int64)
    overlap[1, 1, 1], overlap[1, 1, 2] = 5, 5                                                  # a tie: b = 1, id 1 (2 * 5 >= min(9, 10))
    overlap[1, 3, 1], overlap[1, 3, 2] = 9, 4                                                  # b = 1 is taken: b = 2, 2 * 4 >= min(12, 8)
    overlap[2, 1, 1], overlap[2, 1, 3] = 5, 4                                                  # b = 1: 2 * 5 >= min(20, 9) = 9
    overlap[2, 2, 3] = 3                                                                       # 2 * 3 >= min(6, 12) = 6
    overlap[2, 3, 3], overlap[2, 3, 0] = 2, 5                                                  # b = 3 is taken, b = 0 is the camera: new
    overlap[3, 1, 1] = 2                                                                       # 2 * 2 >= min(4, 20) = 4
    overlap[3, 2, 2] = 1                                                                       # 2 * 1 < min(4, 6): new
    overlap[3, 3, 2] = 4                                                                       # b = 2 was not taken: id of pair 2's layer 2
    ids, next_id = drivers.link_layers(head, overlap)
    assert ids.dtype == torch.int64 and ids.tolist() == [[0, 1, 2, -1], [0, 1, -1, 2], [-1, 1, 2, 3], [0, 1, 4, 2]] and next_id == 5
    # the same pairs in two calls: prev_ids and prev_counts carry the state
    first, nid = drivers.link_layers(head[:2], overlap[:2])
    rest, nid = drivers.link_layers(head[2:], overlap[2:], prev_ids=first[-1], prev_counts=head[1, :, 1], next_id=nid)
    assert torch.cat([first, rest]).tolist() == ids.tolist() and nid == 5
    # without prev_ids the first pair links against nothing, and ids start at next_id
    alone, nid = drivers.link_layers(head[2:], overlap[2:], next_id=7)
    assert alone.tolist() == [[-1, 7, 8, 9], [0, 7, 10, 8]] and nid == 11
    # zero overlap never inherits; an id of -1 before is no candidate
    head = _head([[9, 5, None], [9, 5, 5]])
    overlap = torch.zeros(2, 3, 3, dtype=torch.int64)
    overlap[1, 2, 2] = 5
    assert drivers.link_layers(head, overlap)[0].tolist() == [[0, 1, -1], [0, 2, 3]]
    assert drivers.link_layers(torch.zeros(0, 3, 4), torch.zeros(0, 3, 3))[0].shape == (0, 3)
    for bad in (dict(prev_ids=[0, 1, 2]), dict(prev_ids=[0, 1], prev_counts=[1, 2]), dict(next_id=0)):
        with pytest.raises(ValueError):
            drivers.link_layers(head, overlap, **bad)
    with pytest.raises(ValueError):
        drivers.link_layers(head, overlap[:, :2])


# ---------------------------------------------------------------------------------------------- the drivers
def test_driver_returns_the_tables_and_ids_sort_the_columns():
    trajs, g = _scene(5, 60, 8, outliers=0.4), torch.Generator().manual_seed(8)
    vis = torch.randn(5, 60, generator=g) + 1.5
    logit = float(torch.logit(torch.tensor(0.7, dtype=torch.float32)))
    head, _, model, box, layer, overlap = drivers.motion_layers_table_torch(trajs, vis, 11, logit, 32, 6, 99, 3, 2)
    kw = dict(frame0=11, thr=1.5, hypotheses=32, vis_thr=0.7, seed=99, layers=3, min_inliers=2)
    models, counts, labels, object_ids, objects, boxes = drivers.motion_layers_torch(trajs[None], vis[None], **kw)
    assert models.dtype == torch.float64 and _f64_bits(models) == _f64_bits(model) and counts.tolist() == head[:, :, :2].tolist()
    assert labels.dtype == torch.int64 and torch.equal(labels == -2, layer == 255) and torch.equal(labels == -1, layer == 254)
    assert torch.equal(labels[labels >= 0], layer[layer < 3].long()) and int((labels >= 1).sum()) > 6
    ids, next_id = drivers.link_layers(head, overlap)
    assert torch.equal(object_ids, ids) and next_id > 1 and boxes.dtype == torch.float64 and torch.equal(boxes, box.double() / 4.0)
    for f in range(4):
        for k in range(60):
            want = int(labels[f, k]) if labels[f, k] < 0 else int(ids[f, int(labels[f, k])])
            assert int(objects[f, k]) == want
    perm = torch.randperm(60, generator=g)
    got = drivers.motion_layers_torch(trajs[None][:, :, perm], vis[None][:, :, perm], ids=perm, **kw)
    assert _f64_bits(got[0]) == _f64_bits(models) and torch.equal(got[1], counts) and torch.equal(got[2], labels[:, perm])
    assert torch.equal(got[3], object_ids) and torch.equal(got[4], objects[:, perm]) and torch.equal(got[5], boxes)


@pytest.mark.parametrize("with_vis", [False, True])
@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_layers_push_by_push_are_the_whole_video_call(chunk, with_vis):
    """T = 19, 40 identities that are born and retired on the way; a push holds the identities alive in it, in a shuffled order of
    their own: labels, objects, models and ids of every pair equal those of one call on the video by identity"""
    T, K = 19, 40
    trajs, vis, born, last = _life_video(T, K, 21)
    kw = dict(thr=1.5, hypotheses=48, vis_thr=0.6, seed=5, layers=4, min_inliers=2)
    whole = drivers.motion_layers_torch(trajs[None], vis[None] if with_vis else None, ids=torch.arange(K), **kw)
    assert int(whole[3].max()) >= 4 and int((whole[3][1:] >= 1).sum()) > 8                     # objects are found, ids are handed on
    inherited = sum(int(i) in whole[3][f - 1].tolist() for f in range(1, T - 1) for i in whole[3][f].tolist() if i >= 1)
    assert inherited >= 1
    ml = drivers.MotionLayers(engine="torch", **kw)
    g = torch.Generator().manual_seed(22)
    got, pair = [], 0
    assert ml.step(0, trajs[None][:, :0, :0])[0].shape == (0, 4, 4)                            # a push without rows
    for f0 in range(0, T, chunk):
        f1 = min(f0 + chunk, T)
        alive = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
        ids = alive[torch.randperm(alive.numel(), generator=g)]
        out = ml.step(f0, trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids] if with_vis else None, ids=ids)
        P = f1 - f0 - (1 if f0 == 0 else 0)
        assert tuple(out[0].shape) == (P, 4, 4) and tuple(out[2].shape) == (P, ids.numel()) and ml.T == f1
        assert _f64_bits(out[0]) == _f64_bits(whole[0][pair:pair + P]) and torch.equal(out[1], whole[1][pair:pair + P])
        assert torch.equal(out[2], whole[2][pair:pair + P][:, ids]) and torch.equal(out[3], whole[3][pair:pair + P])
        assert torch.equal(out[4], whole[4][pair:pair + P][:, ids]) and torch.equal(out[5], whole[5][pair:pair + P])
        assert int((whole[2][pair:pair + P] >= 0).sum()) == int((out[2] >= 0).sum())           # nobody outside the push has a label
        got.append(out[3])
        pair += P
    assert pair == T - 1 and ml.next_id == int(whole[3].max()) + 1
    with pytest.raises(ValueError):
        ml.step(T + 1, trajs[None][:, :1])                                                     # a gap
    with pytest.raises(ValueError):
        ml.step(T, trajs[None][:, :1, :5], ids=[0, 1, 2, 3])
    with pytest.raises(ValueError):
        ml.step(T, trajs[None][:, :1], None if with_vis else vis[None][:, :1])                 # vis on every step or on none
    with pytest.raises(ValueError):
        ml.step(T, trajs[None][:, :1, :ids.numel()], vis[None][:, :1, :ids.numel()] if with_vis else None)   # ids on every step or on none


def test_layers_with_stable_columns_need_no_ids():
    trajs = _scene(9, 25, 31, outliers=0.4)
    kw = dict(hypotheses=32, seed=3, layers=3, min_inliers=2)
    whole = drivers.motion_layers_torch(trajs[None], **kw)
    ml = drivers.MotionLayers(engine="torch", **kw)
    parts = [ml.step(f0, trajs[None][:, f0:f0 + 4]) for f0 in range(0, 9, 4)]
    for k in range(6):
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
    with pytest.raises(ValueError):
        ml.step(9, trajs[None][:, :1, :20])                                                    # the columns changed without ids
    with pytest.raises(ValueError):
        ml.step(9, trajs[None][:, :1], ids=torch.arange(25))                                   # ids after steps without


# ---------------------------------------------------------------------------------------------- what the layers mean
SCENE_SHIFTS = ((14.0, 0.0), (0.0, -15.0))                               # px a frame; 14, 15 and 20.5 apart: >= 6 x thr = 12
SCENE_SEEDS = {64: 2, 200: 10}                                         # seeds on which the plain-loop reference meets the conditions


def _meaning_scene(n, seed, F=6):
    """60 % of the columns follow the camera (``_scene``'s similarity a frame, +-0.25 px noise); two compact blobs of 20 % and 12 %
    follow the camera plus a constant shift of their own a frame; 8 % go ways of their own; the columns are shuffled -> (trajs
    (F,n,2) float32, group (n,) = 0 camera, 1 and 2 the blobs, 3 wild)"""
    g = torch.Generator().manual_seed(seed)
    D = torch.float64
    sizes = [round(0.2 * n), round(0.12 * n), round(0.08 * n)]
    group = torch.cat([torch.zeros(n - sum(sizes)), torch.ones(sizes[0]), torch.full((sizes[1],), 2.0), torch.full((sizes[2],), 3.0)]).long()
    p = torch.rand(n, 2, generator=g, dtype=D) * torch.tensor([640.0, 480.0], dtype=D)
    for b, centre in ((1, (160.0, 330.0)), (2, (470.0, 300.0))):
        at = group == b
        p[at] = torch.tensor(centre, dtype=D) + (torch.rand(int(at.sum()), 2, generator=g, dtype=D) - 0.5) * 90.0
    rows = [p]
    for _ in range(1, F):
        ang, sc = (torch.rand(2, generator=g, dtype=D) - 0.5) * torch.tensor([math.radians(6.0), 0.06], dtype=D)
        a = (1.0 + float(sc)) * complex(math.cos(float(ang)), math.sin(float(ang)))
        t = (torch.rand(2, generator=g, dtype=D) - 0.5) * 24.0
        p = rows[-1]
        q = torch.stack([a.real * p[:, 0] - a.imag * p[:, 1], a.imag * p[:, 0] + a.real * p[:, 1]], dim=1) + t
        q = q + (torch.rand(n, 2, generator=g, dtype=D) - 0.5) * 0.5
        for b, shift in ((1, SCENE_SHIFTS[0]), (2, SCENE_SHIFTS[1])):
            q[group == b] += torch.tensor(shift, dtype=D)
        wild = group == 3
        q[wild] += (torch.rand(int(wild.sum()), 2, generator=g, dtype=D) - 0.5) * 120.0
        rows.append(q)
    perm = torch.randperm(n, generator=g)
    return torch.stack(rows).to(torch.float32)[:, perm], group[perm]


def _scene_conditions(labels, object_ids, group):
    """each group carries one label per pair (the camera layer 0, the blobs a layer of their own each), each blob keeps one object
    id over all pairs, at most 2 % of the wild columns are labelled"""
    P = len(labels)
    blob_ids = {1: set(), 2: set()}
    for f in range(P):
        seen = []
        for b in (0, 1, 2):
            mine = {labels[f][k] for k in range(len(group)) if group[k] == b}
            if len(mine) != 1 or min(mine) < 0:
                return False
            seen.append(mine.pop())
            if b:
                blob_ids[b].add(object_ids[f][seen[-1]])
        if seen[0] != 0 or len(set(seen)) != 3:
            return False
    wild = [labels[f][k] for f in range(P) for k in range(len(group)) if group[k] == 3]
    return all(len(s) == 1 and min(s) >= 1 for s in blob_ids.values()) and blob_ids[1] != blob_ids[2] and \
        sum(x >= 0 for x in wild) <= 0.02 * len(wild)


@pytest.mark.parametrize("n", [64, 200])
def test_a_scene_with_a_camera_two_blobs_and_wild_columns(n):
    """6 rows, K = 256, thr4 = 8, L = 4, min_inliers = 8.  The plain-loop reference is run first and must meet the conditions on the
    chosen seed itself; then the driver must."""
    trajs, group = _meaning_scene(n, SCENE_SEEDS[n])
    shifts = [torch.tensor(s) for s in SCENE_SHIFTS]
    assert min(float(shifts[0].norm()), float(shifts[1].norm()), float((shifts[0] - shifts[1]).norm())) >= 6 * 2.0
    assert [int((group == b).sum()) for b in range(4)] == [n - round(0.2 * n) - round(0.12 * n) - round(0.08 * n), round(0.2 * n),
                                                           round(0.12 * n), round(0.08 * n)]
    vis_logit = float(torch.logit(torch.tensor(0.5, dtype=torch.float32)))
    ref = _layers_rule(trajs, None, 0, vis_logit, 256, 8, 0, 4, 8)
    ref_ids, _ = drivers.link_layers(torch.tensor(ref[0]), torch.tensor(ref[5]))
    ref_labels = [[-2 if x == 255 else -1 if x == 254 else x for x in row] for row in ref[4]]
    assert _scene_conditions(ref_labels, ref_ids.tolist(), group.tolist())                     # the condition: the reference itself
    models, counts, labels, object_ids, objects, boxes = drivers.motion_layers_torch(trajs[None], thr=2.0, hypotheses=256, seed=0,
                                                                                    layers=4, min_inliers=8)
    assert _scene_conditions(labels.tolist(), object_ids.tolist(), group.tolist())
    assert labels.tolist() == ref_labels and object_ids.tolist() == ref_ids.tolist()
    for b in (1, 2):                                                                           # a blob's columns carry its id, and its
        ident = int(objects[0][group == b][0])                                                 # box holds them
        assert ident >= 1 and bool((objects[:, group == b] == ident).all())
        for f in range(5):
            l = int(labels[f][group == b][0])
            inside = trajs[f + 1][group == b]
            assert bool((inside[:, 0] >= boxes[f, l, 0] - 0.125).all() and (inside[:, 0] <= boxes[f, l, 2] + 0.125).all())
            assert bool((inside[:, 1] >= boxes[f, l, 1] - 0.125).all() and (inside[:, 1] <= boxes[f, l, 3] + 0.125).all())


# ---------------------------------------------------------------------------------------------- bad arguments, the ABI
def test_bad_arguments_are_rejected():
    t = torch.zeros(3, 4, 2)
    good = dict(frame0=0, K=8, thr4=8, seed=0, L=2, min_in=2)
    for bad in (dict(K=0), dict(K=1025), dict(thr4=0), dict(thr4=1025), dict(frame0=-1), dict(frame0=2 ** 31 - 3), dict(seed=-1),
                dict(seed=2 ** 32), dict(L=0), dict(L=9), dict(min_in=1), dict(min_in=65537)):
        a = dict(good, **bad)
        with pytest.raises(ValueError):
            drivers.motion_layers_table_torch(t, None, a["frame0"], 0.0, a["K"], a["thr4"], a["seed"], a["L"], a["min_in"])
    for shape in ((3, 4), (3, 4, 3)):
        with pytest.raises(ValueError):
            drivers.motion_layers_table_torch(torch.zeros(shape), None, 0, 0.0, 8, 8, 0, 2, 2)
    with pytest.raises(ValueError):
        drivers.motion_layers_table_torch(t, torch.zeros(3, 5), 0, 0.0, 8, 8, 0, 2, 2)
    with pytest.raises(ValueError):
        drivers.motion_layers_table_torch(t, None, 0, 0.0, 8, 8, 0, 2, 2, torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        drivers.motion_layers_table_torch(t, None, 0, 0.0, 8, 8, 0, 2, 2, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        drivers.motion_layers_table_torch(torch.zeros(2, 65537, 2), None, 0, 0.0, 8, 8, 0, 2, 2)
    t4 = t.unsqueeze(0)
    for bad in (dict(thr=0.3), dict(thr=True), dict(hypotheses=0), dict(hypotheses=1025), dict(vis_thr=0.0), dict(seed=-1),
                dict(layers=0), dict(layers=9), dict(layers=2.5), dict(layers=True), dict(min_inliers=1), dict(min_inliers=65537),
                dict(frame0=-1), dict(ids=[0, 1, 2]), dict(ids=[0, 1, 2, 2])):
        with pytest.raises(ValueError):
            drivers.motion_layers_torch(t4, **bad)
        if "ids" not in bad and "frame0" not in bad:
            with pytest.raises(ValueError):
                drivers.MotionLayers(engine="torch", **bad)
    with pytest.raises(ValueError):
        drivers.motion_layers_torch(t)
    with pytest.raises(ValueError):
        drivers.motion_layers_torch(t4, vis=torch.zeros(1, 3, 5))
    with pytest.raises(ValueError):
        drivers.MotionLayers(engine="cpu")
    with pytest.raises(ValueError):
        drivers.MotionLayers(engine="torch", trail=3)
    out = drivers.motion_layers_torch(t4, layers=8, min_inliers=2)
    assert [tuple(o.shape) for o in out] == [(2, 8, 4), (2, 8, 2), (2, 4), (2, 8), (2, 4), (2, 8, 4)]


def test_motion_layers_is_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    still = re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)                # the history comment
    assert "pips_motion_layers" in still and "pips_motion_layers_workspace_bytes" in still
    for words in ("0x632BE5AB", "seed_0 = seed", "need_0 = 2", "min_in", "Without a model nothing leaves", "no early stop",
                  "255 for a column that is not valid", "254 for a valid column in no layer", "prev_layer", "min qx, min qy",
                  "24 n + 4 (1 + ceil(K / 64))", "no memory beyond one pair"):
        assert words in hdr, words                                         # the rule stands in the header
    assert int(re.search(r"#define PIPS_MOTION_LAYERS_MAX\s+(\d+)", hdr).group(1)) == ops.MOTION_LAYERS_MAX == 8
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_motion_layers\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 21
    proto = re.search(r"\bsize_t\s+pips_motion_layers_workspace_bytes\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 4
    res, args = _lib.SIGNATURES["pips_motion_layers"]
    assert res is ctypes.c_int and len(args) == 21 and args[6] is ctypes.c_float and args[9] is ctypes.c_int
    assert args[19] is ctypes.c_size_t
    assert _lib.SIGNATURES["pips_motion_layers_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert "motion.hip" in _build.SOURCES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_motion_layers") and hasattr(raw, "pips_motion_layers_workspace_bytes")
    assert callable(ops.motion_layers) and callable(ops.motion_layers_workspace_bytes)
    for name in ("motion_layers", "motion_layers_torch", "motion_layers_table_torch", "link_layers", "MotionLayers"):
        assert callable(getattr(drivers, name)), name
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the sizing query is a host function: per pair two lists of 12 bytes a column, the count and a key per block of 64 hypotheses
    size = lib.pips_motion_layers_workspace_bytes
    assert size(5, 100, 256, 4) == 4 * (2400 + 4 * 5) and size(2, 1, 1, 1) == 24 + 8 and size(2, 65536, 1024, 8) == 24 * 65536 + 4 * 17
    assert size(3, 7, 64, 1) == size(3, 7, 64, 8) == 2 * (168 + 8) and size(3, 7, 65, 2) == 2 * (168 + 12)
    assert ops.motion_layers_workspace_bytes(3, 7, 65, 2) == 360
    assert size(1, 100, 64, 4) == 0 and size(0, 100, 64, 4) == 0 and size(5, 0, 64, 4) == 0
    assert size(-1, 8, 8, 4) == 0 and size(5, -1, 8, 4) == 0 and size(5, 65537, 8, 4) == 0 and size(5, 8, 0, 4) == 0
    assert size(5, 8, 1025, 4) == 0 and size(5, 8, 8, 0) == 0 and size(5, 8, 8, 9) == 0
    assert size((1 << 24) + 1, 8, 8, 4) == 0 and size(1 << 24, 8, 8, 4) > 0
    # the host-side rejections need no device: nothing is launched

    def call(F=3, n=8, frame0=0, logit=0.0, K=8, thr4=8, L=4, min_in=8):
        return lib.pips_motion_layers(None, None, None, F, n, frame0, logit, K, thr4, 0, L, min_in, None, None, None, None, None, None,
                                      None, 0, None)

    for bad in (dict(F=-1), dict(F=(1 << 24) + 1), dict(n=-1), dict(n=65537), dict(K=0), dict(K=1025), dict(thr4=0), dict(thr4=1025),
                dict(frame0=-1), dict(frame0=2 ** 31 - 3), dict(logit=NAN), dict(L=0), dict(L=9), dict(min_in=1), dict(min_in=65537),
                dict()):
        assert call(**bad) == -1, bad
        assert lib.pips_last_error().decode().startswith("motion_layers:"), bad
    assert call(F=0) == 0 and call(F=1) == 0 and call(F=1, n=0) == 0                           # nothing to fit, nothing launched
