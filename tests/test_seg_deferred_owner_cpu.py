"""Deferred segmentation on a sharded map without a GPU: the new C-ABI entries are declared and bound, and the per-rank translation statement
(tests/seg_deferred_owner_numpy.py) splits the unsharded translation (tests/seg_deferred_numpy.py) among the ranks: on random shards the ranks' kept pixels are
disjoint and their union is the merged map's."""
import re

import numpy as np
import pytest

from seg_deferred_numpy import translate_ids
from seg_deferred_owner_numpy import lost_owner, translate_ids_owner

ENTRIES = ("ifx_owner_segmentation_snapshot", "ifx_owner_segmentation_begin_deferred", "ifx_owner_segmentation_begin_deferred_device",
           "ifx_owner_process_segmentation_deferred", "ifx_owner_process_segmentation_deferred_device")


def test_header_declares_and_binding_covers_the_entries():
    import instancefusion_amd as m
    from instancefusion_amd import sharded

    header = open(m.HEADER_PATH).read()
    bound = m.exported_symbols()
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(\s*ifx_t\s*\*\s*h\b([^;]*)\);", header)
        assert decl, name
        assert name in bound, name
        assert len(m._SIGS[name][1]) == decl.group(1).count(",") + 1, name
    for meth in ("snapshot", "process_segmentation_deferred", "process_segmentation_deferred_device", "release_snapshot", "snapshot_stats"):
        assert callable(getattr(sharded.OwnerShardedElasticFusion, meth)), meth
    for fn in ("emulate_owner_snapshot", "emulate_owner_segmentation_deferred", "emulate_owner_segmentation_deferred_device"):
        assert callable(getattr(sharded, fn)), fn


def test_statement_on_a_hand_made_shard():
    # this rank stores 4 (alive), 7 (a tombstone), 9 and 15 (alive); 4 is the lowest live number of any rank; 5 and 11 live on another rank; 6 is gone everywhere
    seq = np.array([4, 7, 9, 15], np.uint32)
    alive = np.array([True, False, True, True])
    pinned = np.array([[0, 4, 5, 6], [7, 9, 11, 15]], np.int32)
    assert translate_ids_owner(pinned, seq, alive, 4).tolist() == [[0, 0, 0, 0], [0, 3, 0, 4]]
    # the same shard when a lower number is alive on another rank: slot 0 is an ordinary surfel and reads 1
    assert translate_ids_owner(pinned, seq, alive, 2).tolist() == [[0, 1, 0, 0], [0, 3, 0, 4]]
    # numbers from 2^31 on travel in the int32 image as negative values
    big = np.array([0x80000005, 0xFFF00000 - 1], np.uint32)
    assert translate_ids_owner(big.view(np.int32), big, np.array([True, True]), 1).tolist() == [1, 2]
    assert translate_ids_owner(pinned, np.zeros(0, np.uint32), np.zeros(0, bool), 4).tolist() == [[0] * 4, [0] * 4]
    assert lost_owner(pinned, np.array([4, 6, 7, 9, 15], np.uint32), seq, alive, 2) == 2      # 6 (gone) and 7 (dead); 4, 9, 15 kept; 5 and 11 were never this rank's


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_ranks_split_the_unsharded_translation(G, seed):
    rng = np.random.default_rng(10 * G + seed)
    n_then = 4000
    seq_then = np.cumsum(rng.integers(1, 4, n_then)).astype(np.uint32)           # ascending creation numbers of the compact map at the snapshot
    owner = {int(s): int(rng.integers(0, G)) for s in seq_then}
    ids_then = rng.integers(0, n_then, (60, 80)).astype(np.int32)                # slots of the unsharded image; 0 = no surfel (the first live surfel is never drawn)
    ids_then[rng.random(ids_then.shape) < 0.2] = 0
    pinned = np.where(ids_then > 0, seq_then[ids_then], 0).astype(np.uint32).view(np.int32)
    # now: a third of the surfels died (some of them, seed 0, from the front: "surfel 0" moves up), new ones were created behind
    dead = rng.random(n_then) < 0.33
    if seed == 0:
        dead[:5] = True
    new = (int(seq_then[-1]) + np.cumsum(rng.integers(1, 4, 500))).astype(np.uint32)
    for s in new:
        owner[int(s)] = int(rng.integers(0, G))
    seq_now = np.concatenate([seq_then[~dead], new])
    merged = translate_ids(ids_then, seq_then, seq_now)
    surfel0 = int(seq_now[0])
    # a rank's shard keeps a random half of its dead surfels as tombstones (no compaction since): stored, not alive
    kept_any = np.zeros(ids_then.shape, bool)
    lost_sum = 0
    for r in range(G):
        mine_then = np.array([owner[int(s)] == r for s in seq_then])
        stored = mine_then & (~dead | (rng.random(n_then) < 0.5))
        seq_r = np.concatenate([seq_then[stored], new[[owner[int(s)] == r for s in new]]])
        alive_r = np.concatenate([~dead[stored], np.ones(seq_r.size - int(stored.sum()), bool)])
        T = translate_ids_owner(pinned, seq_r, alive_r, surfel0)
        kept = T > 0
        assert not (kept & kept_any).any(), r                                      # disjoint
        kept_any |= kept
        assert np.array_equal(seq_r[T[kept] - 1], seq_now[merged[kept]]), r        # ... and the slot holds the surfel the merged map holds there
        lost_sum += lost_owner(pinned, seq_then[mine_then], seq_r, alive_r, surfel0)
    assert np.array_equal(kept_any, merged > 0)                                    # the union is the unsharded translation
    assert lost_sum == int(((ids_then > 0) & (merged == 0)).sum())
    assert (merged > 0).sum() > 1000 and ((ids_then > 0) & (merged == 0)).sum() > 500
