"""CPU: the host side of the chaining entry points -- the threshold table of the library's skip scan, the workspace query, and
the ``engine`` keyword of the drivers and of their sharded forms.  No GPU calls."""
import pytest
import torch


def test_threshold_table_is_bit_equal_to_the_drivers():
    """pips_chain_threshold(k): 0.9 lowered k times by 0.02 in double, rounded to fp32 -- the 64 values of
    drivers._threshold_table(), bit for bit (the C++ table is built by the same repeated subtraction)."""
    from pips_amd import drivers, ops
    got, want = ops.chain_thresholds(), drivers._threshold_table()
    assert got.dtype == want.dtype == torch.float32 and got.numel() == want.numel() == 64
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # not the same numbers as the closed form in fp32 arithmetic (what a kernel-side 0.9f - 0.02f * k would give)
    closed = torch.tensor(0.9) - torch.tensor(0.02) * torch.arange(64, dtype=torch.float32)
    assert not torch.equal(closed, want)
    from pips_amd import _lib
    lib = _lib.load()
    assert lib.pips_chain_threshold(-1) == 0.0 and lib.pips_chain_threshold(64) == 0.0


def test_chain_workspace_covers_the_tracker_and_the_staging_arrays():
    from pips_amd import _lib
    lib = _lib.load()
    for n_act, iters in ((1, 0), (23, 6), (2500, 6)):
        track = lib.pips_track_workspace_bytes_s(1, n_act, 8)
        staging = 4 * n_act * (2 + 1 + 1 + 128 + (iters + 1) * 16 + 8 + 128)
        assert lib.pips_chain_workspace_bytes(n_act, iters) >= track + staging
        assert lib.pips_chain_workspace_bytes(n_act, iters) < track + 2 * staging + 8 * 256
    assert lib.pips_chain_workspace_bytes(0, 6) == 0 and lib.pips_chain_workspace_bytes(-3, 6) == 0
    assert lib.pips_chain_workspace_bytes(8, -1) == 0
    assert lib.pips_chain_workspace_bytes(64, 6) > lib.pips_chain_workspace_bytes(64, 3)
    assert lib.pips_abi_version() == 3                                   # additions only


def test_engine_keyword_is_validated_and_defaults_to_torch():
    import inspect
    from pips_amd import Pips, dist, drivers
    for fn in (drivers.track_chained, drivers.track_queries, drivers.track_stream, drivers.StreamTracker.__init__,
               dist.track_chained_sharded, dist.track_queries_sharded):
        assert inspect.signature(fn).parameters["engine"].default == "torch", fn
    m = Pips()
    q = torch.zeros(1, 2, 3)
    with pytest.raises(ValueError, match="engine"):
        drivers.track_chained(m, torch.zeros(1, 9, 3, 64, 64), torch.zeros(1, 2, 2), engine="hip")
    with pytest.raises(ValueError, match="engine"):
        drivers.track_queries(m, torch.zeros(1, 9, 3, 64, 64), q, engine="")
    with pytest.raises(ValueError, match="engine"):
        drivers.StreamTracker(m, q, engine="Native")
    assert drivers.StreamTracker(m, q, engine="native").engine == "native"


def test_sharded_drivers_pass_the_engine_through(monkeypatch):
    from pips_amd import dist, drivers
    seen = []

    def chained(model, rgbs, xy0, iters=6, return_hops=False, engine="torch"):
        seen.append(("chained", engine))
        return torch.zeros(1, rgbs.shape[1], xy0.shape[1], 2)

    def queries(model, rgbs, q, iters=6, return_hops=False, engine="torch"):
        seen.append(("queries", engine))
        return torch.zeros(1, rgbs.shape[1], q.shape[1], 2), torch.zeros(1, rgbs.shape[1], q.shape[1])

    monkeypatch.setattr(drivers, "track_chained", chained)
    monkeypatch.setattr(drivers, "track_queries", queries)
    rgbs = torch.zeros(1, 9, 3, 8, 8)
    dist.track_chained_sharded(None, rgbs, torch.zeros(1, 4, 2), engine="native")
    dist.track_queries_sharded(None, rgbs, torch.zeros(1, 4, 3), engine="native")
    dist.track_chained_sharded(None, rgbs, torch.zeros(1, 4, 2))
    assert seen == [("chained", "native"), ("queries", "native"), ("chained", "torch")]
