"""Reference for the ID mattes (vk_render_mattes, vk_matte_merge, vk_matte_mask), written from the text of include/vecchio_amd.h alone:
the table of a pixel, the merge of two tables and the mask, in plain Python over numpy arrays.  TESTS ONLY."""
import numpy as np

BACKGROUND = 0xFFFFFFFF
MAX_RANKS = 8


def _insert(slots, ranks, ident, c):
    """found: add; a free slot: take it; else the overflow.  slots: a list of [id, count] in the order they were taken"""
    for s in slots:
        if s[0] == ident:
            s[1] += c
            return 0
    if len(slots) < ranks:
        slots.append([ident, c])
        return 0
    return c


def _write(slots, ranks):
    """count descending, ties by id ascending; an unused slot is (0, 0)"""
    slots = sorted(slots, key=lambda s: (-s[1], s[0]))
    ids = [s[0] for s in slots] + [0] * (ranks - len(slots))
    counts = [s[1] for s in slots] + [0] * (ranks - len(slots))
    return ids, counts


def table(sample_ids, ranks):
    """sample_ids (..., n) in increasing sample order -> ids (..., ranks), counts (..., ranks), overflow (...), all uint32"""
    assert 1 <= ranks <= MAX_RANKS
    sample_ids = np.asarray(sample_ids, np.uint32)
    flat = sample_ids.reshape(-1, sample_ids.shape[-1])
    ids = np.zeros((len(flat), ranks), np.uint32)
    counts = np.zeros((len(flat), ranks), np.uint32)
    overflow = np.zeros(len(flat), np.uint32)
    for i, row in enumerate(flat.tolist()):
        slots, over = [], 0
        for ident in row:
            over += _insert(slots, ranks, ident, 1)
        ids[i], counts[i] = _write(slots, ranks)
        overflow[i] = over
    shape = sample_ids.shape[:-1]
    return ids.reshape(shape + (ranks,)), counts.reshape(shape + (ranks,)), overflow.reshape(shape)


def merge(a, b):
    """table b folded into table a: (ids, counts, overflow) each; b's used slots in b's order, then overflow += overflow_b, sorted again.
    Returns new arrays."""
    ids_a, counts_a, over_a = a
    ids_b, counts_b, over_b = b
    ranks = ids_a.shape[-1]
    assert ids_b.shape == ids_a.shape and 1 <= ranks <= MAX_RANKS
    fa, ca = ids_a.reshape(-1, ranks).tolist(), counts_a.reshape(-1, ranks).tolist()
    fb, cb = ids_b.reshape(-1, ranks).tolist(), counts_b.reshape(-1, ranks).tolist()
    ids = np.zeros((len(fa), ranks), np.uint32)
    counts = np.zeros((len(fa), ranks), np.uint32)
    overflow = np.asarray(over_a, np.uint32).reshape(-1).astype(np.uint64) + np.asarray(over_b, np.uint32).reshape(-1)
    for i in range(len(fa)):
        slots = [[fa[i][r], ca[i][r]] for r in range(ranks) if ca[i][r] != 0]
        for r in range(ranks):
            if cb[i][r] != 0:
                overflow[i] += _insert(slots, ranks, fb[i][r], cb[i][r])
        ids[i], counts[i] = _write(slots, ranks)
    return ids.reshape(ids_a.shape), counts.reshape(ids_a.shape), overflow.astype(np.uint32).reshape(ids_a.shape[:-1])


def mask(ids, counts, n_samples, want):
    """(float)(sum of the counts of the slots whose id is in `want`) / (float)n_samples"""
    want = np.asarray(list(want), np.uint32)
    inside = np.isin(ids, want) & (counts != 0)
    total = np.where(inside, counts, 0).sum(-1, dtype=np.uint64)
    return (total.astype(np.float32) / np.float32(n_samples)).astype(np.float32)
