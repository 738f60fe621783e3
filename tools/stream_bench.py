"""Streamed tracking at the BASELINE configs[4] geometry: drivers.track_stream against track_queries and track_chained.

360x640 frames, stride 4, 256 query points (a 16 x 16 grid) split over frames 0/33/66/99, seeded synthetic uint8 frames made
on the host, chunks of 16 frames, a ring of 24 slots.  Prints one JSON line:
  * wall time of each driver at T = 100 (median of --reps calls after a warm-up; the linear drivers get the video on the
    device, the stream gets host chunks);
  * peak torch.cuda.max_memory_allocated above the pre-call allocation at T = 100 and T = --long (1000), the device video of
    the linear drivers included;
  * the bytes pips_pyramid_append moves per frame (fp32 read + fp32 write + bf16 mirror write), for the kernel-trace run.
The append kernel's time comes from a separate ``rocprofv3 --kernel-trace --stats`` run of ``--only stream``.
``--rounds``: instead, the stream under ``rounds="torch"`` and ``rounds="library"`` (one pips_stream_round call per round) at T,
alternating on one GPU after a warm-up of each, medians of --reps calls; the rounds of one call are counted and the two outputs
compared bit for bit.
``--churn``: instead, a ``StreamTracker(rounds="library")`` over T = 400 frames that starts from 256 queries on frame 0 and, from the
second push on, gets 64 new queries before every push (on the oldest frame not returned yet) -- with the 64 oldest columns taken
away by ``remove_queries`` at the same moment, against the same run without the removals.  Per run: the state's column count after
the last push, the median time of the last five pushes and ``torch.cuda.max_memory_allocated``.  Times: one warm-up of each run, then
--reps of each, alternating on one model, and the medians over those.  Memory: one run of each on a model of its own (a model keeps
the round workspace of the widest state it has served).
``--cover``: instead, a ``CoverTracker(rounds="library")`` over T = 400 frames of the same config that starts from no query of the
caller's: cells of 32 px (a 12 x 20 grid), default policy, ``scan="torch"`` against ``scan="library"``.  Prints the live count per
push (the same under both scans: checked), and per scan the median push time and the median time of the cover step alone (the
tracker's ``book.step`` timed with a device synchronisation on either side).  One warm-up of each, then --reps of each, alternating.
``--seed corners`` seeds on corners (``Cover(seed="corners")``: one corner table per pushed chunk, the seeds of a step placed on it)
instead of on the cell centres (``--min-corner``: the score a corner needs); frames per second (T over the summed push times, the median over the runs) is printed per scan.
``--per-cell K [--crowd-after A]`` thins the cover (``Cover(per_cell=K, crowd_after=A)``: the thin step); the retirements of the
run are counted by reason in every case.
``--cuts K`` makes the synthetic image change K times, at equal distances (another texture in another brightness range: a scene
cut); ``--cut-thr X`` ends the tracks there (``Cover(cut_thr=X)``).  Run both with and without ``--cut-thr`` on the same video: without
it the old scene's tracks stay in their cells and the new scene is seeded only where they happen to fall out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pips_amd import Pips, _lib, drivers  # noqa: E402
from pips_amd.weights import init_state_dict  # noqa: E402

H, W, STRIDE, N, CHUNK, SLOTS = 360, 640, 4, 256, 16, 24


def frames(t0, k, seed=5, cuts=0):
    """frames t0 .. t0+k-1 of a seeded synthetic video (a textured image drifting by one pixel per frame + noise), uint8; with
    ``cuts`` the image changes that many times over the k frames: a new texture, dark (0..102) and bright (150..252) in turn"""
    def image(scene):
        g = torch.Generator().manual_seed(seed + 7919 * scene)
        base = torch.randint(0, 256, (3, H // 8, W // 8), generator=g).float()
        base = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        return base if cuts == 0 else base * 0.4 + 150.0 * (scene % 2)

    bases = [image(s) for s in range(cuts + 1)]
    out = []
    for t in range(t0, t0 + k):
        gt = torch.Generator().manual_seed(seed * 100003 + t)
        base = bases[(t - t0) * (cuts + 1) // k]
        f = torch.roll(base, shifts=(t // 3, t), dims=(1, 2)) + torch.randint(0, 12, (3, H, W), generator=gt).float()
        out.append(f.clamp(0, 255).to(torch.uint8))
    return torch.stack(out).unsqueeze(0)


def chunks(host):
    for t0 in range(0, host.shape[1], CHUNK):
        yield host[:, t0:t0 + CHUNK]


def queries(dev):
    gy, gx = torch.meshgrid(torch.linspace(16, H - 17, 16), torch.linspace(16, W - 17, 16), indexing="ij")
    t = torch.tensor([(0, 33, 66, 99)[n % 4] for n in range(N)], dtype=torch.float32)
    return torch.stack([t, gx.reshape(-1), gy.reshape(-1)], -1).unsqueeze(0).to(dev)


def run(name, m, q, host, video=None, rounds="torch"):
    if name == "stream":
        return drivers.track_stream(m, chunks(host), q, iters=6, slots=SLOTS, rounds=rounds)
    if name == "queries":
        return drivers.track_queries(m, video, q, iters=6)
    return drivers.track_chained(m, video, q[:, :, 1:], iters=6)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - start


def compare_rounds(m, q, host, reps):
    """both values of ``rounds`` on the same chunks -> their median times, the rounds of one call, outputs equal as bit patterns"""
    out, ts = {}, {"torch": [], "library": []}
    count = [0]
    real = m.stream_round

    def counted(*a, **kw):
        count[0] += 1
        return real(*a, **kw)

    m.stream_round = counted
    for mode in ts:                                                     # warm-up: weights, workspaces (and the count)
        out[mode] = run("stream", m, q, host, rounds=mode)
    m.stream_round = real
    for _ in range(reps):
        for mode in ts:
            ts[mode].append(timed(lambda: run("stream", m, q, host, rounds=mode)))
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out["torch"], out["library"]))
    return {"stream_rounds_torch_s": round(statistics.median(ts["torch"]), 4),
            "stream_rounds_library_s": round(statistics.median(ts["library"]), 4), "rounds": count[0], "bit_equal": same}


CHURN_T, CHURN_ADD = 400, 64


def churn_run(m, q0, host, remove):
    """one stream with 64 queries added (and, with ``remove``, the 64 oldest removed) ahead of every push from the second on
    -> (columns of the state after the last push, median seconds of the last five pushes)"""
    dev = q0.device
    st = drivers.StreamTracker(m, q0, iters=6, slots=SLOTS, rounds="library")
    xy = q0[0, :CHURN_ADD, 1:]
    ts = []
    for i, c in enumerate(chunks(host)):
        if i >= 1:
            t = torch.full((CHURN_ADD, 1), float(st.emitted), device=dev)
            st.add_queries(torch.cat([t, xy + float(i % 7)], dim=1).unsqueeze(0))
            if remove:
                st.remove_queries(range(CHURN_ADD))
        ts.append(timed(lambda: st.push(c)))
    cols = st.trajs.shape[1]
    assert cols == st.N
    st.finish()
    torch.cuda.synchronize()
    return cols, statistics.median(ts[-5:])


def compare_churn(dev, q, reps):
    q0 = q.clone()
    q0[0, :, 0] = 0
    host = frames(0, CHURN_T)
    pushes = (CHURN_T + CHUNK - 1) // CHUNK
    runs = {"churn": True, "grow": False}
    res = {"config": "360x640 stride 4, 256 queries on frame 0, chunks of 16, slots 24, library rounds", "T": CHURN_T, "pushes": pushes,
           "added_per_push": CHURN_ADD}
    # memory first, each run on a model of its own: a model keeps the round workspace of the widest state it has served
    for k, remove in runs.items():
        m = model(dev)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        churn_run(m, q0, host, remove)
        res[f"{k}_peak_MiB"] = round(torch.cuda.max_memory_allocated() / 2**20, 1)
        del m
    m = model(dev)
    got = {k: [] for k in runs}
    for k, remove in runs.items():                                      # warm-up: weights, workspaces, the allocator's pools
        churn_run(m, q0, host, remove)
    for _ in range(reps):
        for k, remove in runs.items():
            got[k].append(churn_run(m, q0, host, remove))
    for k, rows in got.items():
        res[f"{k}_columns"] = rows[0][0]
        res[f"{k}_push_ms_last5"] = round(statistics.median(r[1] for r in rows) * 1e3, 2)
    assert res["churn_columns"] == N and res["grow_columns"] == N + CHURN_ADD * (pushes - 1), res
    return res


def cover_run(m, host, scan, seed="centre", min_corner=0, per_cell=None, crowd_after=4, cut_thr=None):
    """one covered stream -> (live count per push, seconds per push, seconds of the cover step of each push that ran one, the
    number of retirements by reason)"""
    cover = drivers.Cover(cell=32, scan=scan, seed=seed, min_corner=min_corner, per_cell=per_cell, crowd_after=crowd_after,
                          cut_thr=cut_thr)
    ct = drivers.CoverTracker(m, cover, None, iters=6, slots=SLOTS, rounds="library")
    steps = []
    real = ct.book.step

    def timed_step(*a, **kw):
        steps.append(timed(lambda: real(*a, **kw)))

    ct.book.step = timed_step
    live, ts = [], []
    for c in chunks(host):
        ts.append(timed(lambda: ct.push(c)))
        live.append(len(ct.book.ids))
    ct.finish()
    torch.cuda.synchronize()
    why = [r for _, r in ct.retired.values()]
    # (steps[0]: the first step, inside the first push)
    return live, ts, steps[1:], dict({r: why.count(r) for r in ("outside", "lost", "crowded", "cut")}, cuts=ct.cuts)


def compare_cover(dev, reps, seed="centre", min_corner=0, per_cell=None, crowd_after=4, cuts=0, cut_thr=None):
    host = frames(0, CHURN_T, cuts=cuts)
    m = model(dev)
    scans = ("torch", "library")
    got = {k: [] for k in scans}
    for k in scans:                                                     # warm-up: weights, workspaces, the allocator's pools
        cover_run(m, host, k, seed, min_corner, per_cell, crowd_after, cut_thr)
    for _ in range(reps):
        for k in scans:
            got[k].append(cover_run(m, host, k, seed, min_corner, per_cell, crowd_after, cut_thr))
    live, retired = got["torch"][0][0], got["torch"][0][3]
    assert all(r[0] == live and r[3] == retired for rows in got.values() for r in rows), "the two scans kept different queries"
    res = {"config": "360x640 stride 4, no caller queries, cell 32 (12 x 20), chunks of 16, slots 24, library rounds", "T": CHURN_T,
           "seed": seed, "min_corner": min_corner, "per_cell": per_cell, "crowd_after": crowd_after if per_cell is not None else None,
           "image_changes_before": [(j * CHURN_T + cuts) // (cuts + 1) for j in range(1, cuts + 1)], "cut_thr": cut_thr,
           "pushes": len(live), "live_per_push": live, "retired": retired}
    for k, rows in got.items():
        res[f"{k}_push_ms"] = round(statistics.median(t for r in rows for t in r[1][2:]) * 1e3, 2)
        res[f"{k}_step_ms"] = round(statistics.median(t for r in rows for t in r[2]) * 1e3, 3)
        res[f"{k}_frames_per_s"] = round(statistics.median(CHURN_T / sum(r[1]) for r in rows), 1)
    return res


def model(dev):
    m = Pips(S=8, stride=STRIDE)
    m.load_state_dict(init_state_dict(0, tamed=True))
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--long", type=int, default=1000, help="video length of the second memory point (0: skip)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="all", choices=["all", "stream"], help="stream: time the stream alone (kernel trace)")
    ap.add_argument("--rounds", action="store_true", help='time rounds="torch" against rounds="library" and nothing else')
    ap.add_argument("--churn", action="store_true", help="queries added and removed at every push against added only, and nothing else")
    ap.add_argument("--cover", action="store_true", help='a covered stream under scan="torch" against scan="library", and nothing else')
    ap.add_argument("--seed", default="centre", choices=list(drivers.COVER_SEEDS), help="with --cover: where in a cell a seed lands")
    ap.add_argument("--min-corner", type=int, default=0, help="with --seed corners: the score a corner needs (above 6372450: the tables "
                    "are made and every seed stays on its centre, which prices the tables alone)")
    ap.add_argument("--per-cell", type=int, default=None, help="with --cover: at most this many tracks to a cell (the thin step)")
    ap.add_argument("--crowd-after", type=int, default=4, help="with --per-cell: surplus frames in a row before a track is retired")
    ap.add_argument("--cuts", type=int, default=0, help="with --cover: the synthetic image changes this many times")
    ap.add_argument("--cut-thr", type=float, default=None, help="with --cover: end the tracks at scene cuts (Cover(cut_thr=))")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.cover:
        print(json.dumps(compare_cover(dev, a.reps, a.seed, a.min_corner, a.per_cell, a.crowd_after, a.cuts, a.cut_thr)))
        return
    q = queries(dev)
    if a.churn:
        print(json.dumps(compare_churn(dev, q, a.reps)))
        return
    m = model(dev)
    names = ["stream"] if a.only == "stream" else ["stream", "queries", "chained"]
    res = {"config": "360x640 stride 4, N=256 over frames 0/33/66/99, chunks of 16, slots 24", "T": a.T}
    host = frames(0, a.T)                                               # host uint8 video: the stream is fed host chunks
    if a.rounds:
        res.update(compare_rounds(m, q, host, a.reps))
        print(json.dumps(res))
        return
    video = None if a.only == "stream" else host.to(dev)
    for name in names:
        run(name, m, q, host, video)                                    # warm-up: weights, workspaces
        ts = [timed(lambda: run(name, m, q, host, video)) for _ in range(a.reps)]
        res[f"{name}_s"] = round(statistics.median(ts), 4)
    del video
    if a.only == "all":
        for T in [a.T] + ([a.long] if a.long else []):
            host = frames(0, T)
            for name in names:
                def call():
                    v = None if name == "stream" else host.to(dev)
                    run(name, m, q, host, v)
                try:
                    res[f"{name}_peak_MiB_T{T}"] = round(peak(call) / 2**20, 1)
                except torch.cuda.OutOfMemoryError:
                    res[f"{name}_peak_MiB_T{T}"] = None
                    torch.cuda.empty_cache()
    lib = _lib.load()
    fl = lib.pips_pyramid_mirror_offset(1, H, W, STRIDE)
    res["pyramid_MiB_per_frame"] = round(lib.pips_pyramid_floats(1, H, W, STRIDE) * 4 / 2**20, 2)
    res["append_bytes_per_frame"] = fl * (4 + 4 + 2)
    res["frames_appended"] = (1 + a.reps) * a.T if "stream" in names else 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
