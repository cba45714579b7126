"""The schedule of a regenerating path batch (vk_regen_*) in numpy, shared by tests/test_regen_emu.py and tests/test_gpu_regen.py.  A
bounce tops the batch up to its capacity with the window's next numbers, every live path ages by one, the expired ones leave, and the
order of the rest stays: which ids are live before and after every bounce is a function of the window's size, the capacity and the
paths' lifetimes alone.  Lifetimes — and whatever belongs to a path at an age: its ray, its state — come from whoever calls: the
emulators, or the window route (vk_film_emit, vk_paths_step one bounce a call) on the device."""
import numpy as np


def schedule(lifetimes, capacity, cull_age=None):
    """lifetimes[q] >= 1: the bounces path q lives, i.e. it retires in its lifetimes[q]-th bounce.  cull_age[q] (0 = never): a rule
    applied between two bounces to the survivors takes path q away once it has survived that many bounces (cull_age[q] < lifetimes[q]
    to have an effect).  Returns one dict per bounce, all uint32 arrays in live order:
      before      the live ids behind the top-up         before_age   the bounces each has behind it (0 for a fresh path)
      after       the survivors of the bounce            after_age    their ages (>= 1)
      retired     the ids the bounce retired, in live order
      culled      the survivors the rule then took, in live order (empty without a rule)
      kept        the survivors it left: the live ids before the next top-up          kept_age"""
    lifetimes = np.asarray(lifetimes, np.int64)
    total = len(lifetimes)
    assert capacity >= 1 and (lifetimes >= 1).all()
    cull_age = np.zeros(total, np.int64) if cull_age is None else np.asarray(cull_age, np.int64)
    u32 = lambda a: np.asarray(a, np.uint32)
    ids, age = np.zeros(0, np.int64), np.zeros(0, np.int64)
    nxt, out = 0, []
    while True:
        m = min(capacity - len(ids), total - nxt)
        ids = np.concatenate([ids, np.arange(nxt, nxt + m)])
        age = np.concatenate([age, np.zeros(m, np.int64)])
        nxt += m
        if len(ids) == 0:
            return out
        b = dict(before=u32(ids), before_age=u32(age))
        age = age + 1
        alive = age < lifetimes[ids]
        b["retired"] = u32(ids[~alive])
        ids, age = ids[alive], age[alive]
        b["after"], b["after_age"] = u32(ids), u32(age)
        gone = cull_age[ids] == age
        b["culled"] = u32(ids[gone])
        ids, age = ids[~gone], age[~gone]
        b["kept"], b["kept_age"] = u32(ids), u32(age)
        out.append(b)


def lifetimes_of(histories, total):
    """histories[a] = the ids live after a bounces of a window stepped whole (histories[0]: all of them): the bounces each path lives"""
    life = np.zeros(total, np.int64)
    for a, ids in enumerate(histories):
        life[np.asarray(ids, np.int64)] = a + 1
    return life


def by_id(histories, arrays, total):
    """arrays[a] = one record per id of histories[a]: per age a an array of `total` records with those at their ids (the rest zero)"""
    out = []
    for ids, arr in zip(histories, arrays):
        full = np.zeros(total, arr.dtype)
        full[np.asarray(ids, np.int64)] = arr
        out.append(full)
    return out
