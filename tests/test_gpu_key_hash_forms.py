"""Key hashing on the plain path (k_hash_keys_ck) in each of its forms: the 20- and 32-byte
instantiations (the message's constant words folded out of round 0), the generic one-block form
(19, 21, 33, 135 bytes) and the multi-block form (136, 200 bytes), all ending in the digest round.
Every root against the CPU batch builder, which hashes the same raw keys itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KLENS = (20, 32, 19, 21, 33, 135, 136, 200)
# one thread, a block and its edges, several blocks; 8,193 and 70,000: the sort that takes the
# kernel's sort words and index, past one radix tile and past the small-sort threshold (65,536)
SIZES = (1, 2, 255, 256, 257, 1000, 8193, 70_000)


def _inputs(klen, n, seed):
    """n distinct random keys of klen bytes, values of 1..8 bytes."""
    r = np.random.default_rng(seed)
    keys = r.integers(0, 256, (n, klen), dtype=np.uint8)
    keys[:, :4] = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4) ^ keys[0, :4]  # distinct
    lens = r.integers(1, 9, n)
    voff = np.zeros(n + 1, np.uint64)
    voff[1:] = np.cumsum(lens)
    vals = r.integers(1, 256, int(voff[-1]) + 8, dtype=np.uint8)
    return keys.reshape(-1), vals, voff


def _dev(*xs):
    import torch
    return [torch.from_numpy(x.astype(np.int64) if x.dtype == np.uint64 else x).to("cuda:0") for x in xs]


@pytest.mark.parametrize("klen", KLENS)
def test_plain_roots_by_key_length(oracle, klen):
    from khipu_amd.device import Ctx
    ctx = Ctx(0)
    for n in SIZES:
        keys, vals, voff = _inputs(klen, n, 1000 * klen + n)
        dk, dv, do = _dev(keys, vals, voff)
        hh, ll, _, st = ctx.build(dk, klen, dv, do, n, hash_keys=True)
        cpu, _ = oracle.batch_roots(keys, (vals, voff), klen=klen, hash_keys=True)
        assert hh[0].tobytes() == cpu[0], (klen, n)
        assert st.n_leaves == n and st.n_key_perms == n * (klen // 136 + 1)


def test_segmented_roots_with_slot_word_keys(oracle):
    """Storage tries (32-byte slot words, a few tries of 1..300 slots): the segmented build's
    launch of the 32-byte instantiation."""
    from khipu_amd.device import Ctx
    cnt = np.array([1, 300, 2, 17, 255, 256, 257, 64, 1, 120], np.int64)
    seg_off = np.zeros(len(cnt) + 1, np.uint64)
    seg_off[1:] = np.cumsum(cnt)
    n = int(seg_off[-1])
    keys, vals, voff = _inputs(32, n, 77)
    seg = np.repeat(np.arange(len(cnt), dtype=np.uint32), cnt)
    dk, dv, do, ds = _dev(keys, vals, voff, seg)
    hh, ll, _, st = Ctx(0).build(dk, 32, dv, do, n, seg=ds, nseg=len(cnt), hash_keys=True)
    cpu, _ = oracle.batch_roots(keys, (vals, voff), klen=32, seg_off=seg_off, hash_keys=True)
    assert [hh[s].tobytes() for s in range(len(cnt))] == cpu
    assert st.n_leaves == n
