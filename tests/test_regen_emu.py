"""The schedule of a regenerating batch on the CPU.  A window stepped whole on the emulators (tests/emu_film_ffi.py emit, the path batch's
emulator loop) gives every path's lifetime and its final state; tests/regen_ref.py schedule() then says which ids are live before and
after every bounce for a capacity.  Checked for capacities on both sides of a wave, of the whole window and beyond it: every path is
emitted exactly once and retired exactly once, live order is ascending at every bounce, the capacity is kept and filled while the window
lasts, and the sums deposited in the schedule's order are tests/film_ref.py's deposit of the whole window.  This pins the reference that
tests/test_gpu_regen.py holds the device against, not the feature."""
import numpy as np
import pytest

import film_ref as F
import regen_ref as G
import shade_ref as S
from vecchio_amd import ffi

SPP = 3
WIN = (3, 2, 11, 7, 0, SPP)                  # 231 paths of the 24 x 16 frame


@pytest.fixture(scope="module")
def stepped(built, host_scenes):
    """the window stepped whole: (frame parameters, lifetimes, final states, statuses, the ids live after every bounce)"""
    import emu_film_ffi
    import emu_paths_ffi
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = ffi.RenderParams.from_buffer_copy(p)
    q.samples_per_pixel, q.max_depth = SPP, 12
    rays, states = emu_film_ffi.emit(cam, q, *WIN)
    b = emu_paths_ffi.Batch(desc, **S.shade_kwargs(q, q.integrator, q.max_depth))
    b.begin(rays, states)
    hist = [b.read()[0]]
    while b.live:
        b.step()
        hist.append(b.read()[0])
    states, status = b.results()
    return q, G.lifetimes_of(hist, len(rays)), states, status, hist


def check(life, capacity, sched):
    total = len(life)
    emitted, retired = np.zeros(total, int), np.zeros(total, int)
    prev_kept, nxt = np.zeros(0, np.uint32), 0
    for b in sched:
        fresh = b["before"][len(prev_kept):]
        assert np.array_equal(b["before"][:len(prev_kept)], prev_kept)                   # the survivors stay in front
        assert np.array_equal(fresh, np.arange(nxt, nxt + len(fresh)))                   # the top-up: the next numbers
        nxt += len(fresh)
        assert len(b["before"]) == min(capacity, len(prev_kept) + total - (nxt - len(fresh)))      # filled while the window lasts
        assert (b["before_age"][len(prev_kept):] == 0).all()
        emitted[fresh] += 1
        retired[b["retired"]] += 1
        retired[b["culled"]] += 1
        for k in ("before", "after", "kept"):
            assert (np.diff(b[k].astype(np.int64)) > 0).all(), k                        # ascending by id
        assert set(b["before"]) == set(b["after"]) | set(b["retired"]) and set(b["after"]) == set(b["kept"]) | set(b["culled"])
        prev_kept = b["kept"]
    assert len(prev_kept) == 0 and nxt == total
    assert (emitted == 1).all() and (retired == 1).all()


@pytest.mark.parametrize("capacity", [1, 64, 65, "total", "total + 7"])
def test_schedule_of_a_window(capacity, stepped):
    q, life, states, status, hist = stepped
    total = len(life)
    assert total == WIN[2] * WIN[3] * WIN[5] and life.max() > 3 and len(set(life.tolist())) > 3
    capacity = {"total": total, "total + 7": total + 7}.get(capacity, capacity)
    sched = G.schedule(life, capacity)
    check(life, capacity, sched)
    # a path retires in the bounce its lifetime names, counted from the bounce that emitted it
    born = np.zeros(total, int)
    for k, b in enumerate(sched):
        born[b["before"][b["before_age"] == 0]] = k
        assert (born[b["retired"]] + life[b["retired"]] == k + 1).all()
    if capacity >= total:
        assert len(sched) == len(hist) - 1                                               # the window route itself
        for b, ids in zip(sched, hist[1:]):
            assert np.array_equal(b["after"], ids)
    else:
        assert len(sched) > len(hist) - 1 and sum(len(b["before"]) for b in sched) == life.sum()
    # the sums, deposited bounce by bounce in the schedule's order
    sums, tot = None, dict(deposited=0, dropped=0, clamped=0, skipped=0)
    for b in sched:
        sums, c = F.deposit(states[b["retired"]], status[b["retired"]], q.width, q.height, SPP, sums)
        tot = {k: tot[k] + c[k] for k in tot}
    want, counters = F.deposit(states, status, q.width, q.height, SPP)
    assert np.array_equal(sums, want) and tot == counters and want.any() and counters["deposited"] + counters["dropped"] == total


def test_schedule_with_a_cull_rule(stepped):
    _, life, _, _, _ = stepped
    total = len(life)
    cull_age = np.where(np.arange(total) % 3 == 1, 2, 0)           # every third path is taken once it has survived two bounces
    hit = (cull_age > 0) & (cull_age < life)
    assert hit.sum() > 5
    for capacity in (1, 64, total + 7):
        sched = G.schedule(life, capacity, cull_age)
        check(life, capacity, sched)
        culled = np.concatenate([b["culled"] for b in sched])
        assert np.array_equal(np.sort(culled), np.flatnonzero(hit))
        for b in sched:
            assert (b["after_age"][np.isin(b["after"], b["culled"])] == 2).all()
