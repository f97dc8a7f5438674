"""CPU: every committed seed of tests/fuzz_cases.py run through the model alone (oracle.Trie plus
the log).  What is asserted here is what keeps tests/test_gpu_commit_fuzz.py from passing emptily:
the sequences reach every edge depth of forest.h's key primitives, make value-only branches, meet
refusals (but not too many), run every operation kind, embed nodes inline and merge an extension
across a 16-nibble word."""
import pytest

from tests import export_cases
from tests import fuzz_cases as F
from tests import partial_cases as P
from tests import writeback as W


def _lcps(keys):
    return [F.lcp(a, b) for a, b in zip(keys, keys[1:])]


def _anchors(keys):
    """{(branch depth, a key under it cut to that depth): the depth its record is anchored at}: one
    past the nearest branch above it (0 at the root), so the extension above a branch at depth db
    covers nibbles [anchor, db)."""
    l = _lcps(keys)
    out = {}
    for i, d in enumerate(l):
        if d == 64:
            continue
        lo = i
        while lo > 0 and l[lo - 1] >= d:
            lo -= 1
        hi = i + 1
        while hi < len(l) and l[hi] >= d:
            hi += 1
        up = max(l[lo - 1] if lo > 0 else -1, l[hi] if hi < len(l) else -1)
        out[(d, keys[i][:d // 2], (keys[i][d // 2] >> 4) if d & 1 else -1)] = up + 1
    return out


def _embedded(enc):
    """The nodes embedded in a node's encoding (lists among a branch's slots or as an extension's target)."""
    it = export_cases._items(enc)
    slots = it[:16] if len(it) == 17 else it[1:2] if len(it) == 2 else []
    n = 0
    for is_list, q, m in slots:
        if is_list:
            n += 1 + _embedded(enc[q - 1:q + m])
    return n


def _stats(seed, oracle):
    s = dict(depths=set(), vb=0, commits=0, refused=0, ops={}, rollback_after_refusal=False, partials=0,
             fetch_after_partial=0, embedded=False, merged=False, steps=[])
    refused_since_save = []
    prev_anchor, after_partial = None, False
    for i, step, m in F.trie_run(seed, oracle):
        s["steps"].append({k: v for k, v in step.items() if k != "side"})
        keys = sorted(m.live)
        s["depths"].update(_lcps(keys))
        op = step["op"]
        s["ops"][op] = s["ops"].get(op, 0) + 1
        if op == "commit":
            s["commits"] += 1
            s["refused"] += step["refused"]
            s["vb"] += bool(step["vb"] and not step["refused"])
            if step["refused"]:
                refused_since_save = [True] * len(refused_since_save)
            if after_partial:
                s["fetch_after_partial"] += bool(step.get("must_fetch"))
                after_partial = False
        anchor = _anchors(keys)
        if op == "commit" and step["dels"] and not step["refused"]:
            for b, a in anchor.items():
                a0 = prev_anchor.get(b, a)
                if a < a0 and any((a < w) != (a0 < w) for w in (16, 32, 48)):
                    s["merged"] = True  # the extension above branch b now starts in an earlier word
        prev_anchor = anchor
        if op == "savepoint":
            refused_since_save.append(False)
        elif op == "release":
            refused_since_save.pop()
        elif op == "rollback":
            s["rollback_after_refusal"] |= refused_since_save.pop()
        elif op == "copy" and step["mode"] == "switch":
            refused_since_save = []
        elif op == "partial":
            s["partials"] += 1
            after_partial = True
        if not s["embedded"] and m.live:
            nodes = m.nodes()
            inline = sum(_embedded(e) for e in nodes.values())
            if inline:
                # reachable() holds fewer nodes than the trie has (len(nodes) + inline): the walk by hash
                # from the root finds exactly the stored ones, the others sit inside their parents
                assert P.subtree(nodes, m.root()) == set(nodes)
                s["embedded"] = True
    return s


@pytest.fixture(scope="module")
def trie_stats(oracle):
    return {seed: _stats(seed, oracle) for seed in F.TRIE_SEEDS}


@pytest.mark.parametrize("seed", F.TRIE_SEEDS)
def test_trie_sequence_covers(trie_stats, seed):
    s = trie_stats[seed]
    assert not set(F.EDGE) - s["depths"], sorted(set(F.EDGE) - s["depths"])
    assert s["vb"] >= 1, "no depth-63 pair re-put"
    assert s["refused"] <= 0.2 * s["commits"], (s["refused"], s["commits"])
    few = [k for k in F.TRIE_OPS if s["ops"].get(k, 0) < 2]
    assert not few, (few, s["ops"])
    assert s["fetch_after_partial"] >= 1, s["partials"]
    assert s["embedded"], "no node embedded inline"
    assert s["merged"], "no extension merged across a 16-nibble word"


def test_trie_sequences_over_the_list(trie_stats):
    assert sum(s["refused"] for s in trie_stats.values()) >= 1
    assert any(s["rollback_after_refusal"] for s in trie_stats.values())


def test_forest_sequences_cover(oracle):
    evicted, loaded, emptied, back, kinds = set(), set(), 0, 0, {}
    for seed in F.FOREST_SEEDS:
        was_empty = set()
        for i, step, ms, resident in F.forest_run(seed, oracle):
            kinds[step["op"]] = kinds.get(step["op"], 0) + 1
            if step["op"] == "evict":
                evicted.update(step["ids"])
            elif step["op"] == "load":
                loaded.update(step["ids"])
            elif step["op"] == "commit" and not step["refused"]:
                now_empty = {t for t in step["touched"] if not ms[t].live}
                back += len({t for t in step["touched"] if ms[t].live} & was_empty)
                emptied += len(now_empty - was_empty)
                was_empty = (was_empty | now_empty) - {t for t in step["touched"] if ms[t].live}
            elif step["op"] == "rollback":
                was_empty = {t for t in was_empty if not ms[t].live}
            assert all(ms[t].root() == W.EMPTY_TRIE_HASH for t in F.FOREST_IDS if not ms[t].live)
    assert evicted == loaded == set(F.FOREST_IDS), (evicted, loaded)
    assert emptied >= 2 and back >= 2, (emptied, back)  # tries taken to empty by a commit, and back
    assert all(kinds.get(k, 0) >= 2 for k in F.FOREST_OPS), kinds


def test_the_generator_is_deterministic(oracle, trie_stats):
    for seed in F.TRIE_SEEDS[:3]:
        assert F.replay(seed, F.NSTEPS + 1, oracle) == trie_stats[seed]["steps"], seed
    assert F.replay(F.TRIE_SEEDS[0], 7, oracle) == trie_stats[F.TRIE_SEEDS[0]]["steps"][:7]
    for seed in F.FOREST_SEEDS[:2]:
        a = [s for _, s, _, _ in F.forest_run(seed, oracle)]
        assert a == [s for _, s, _, _ in F.forest_run(seed, oracle)], seed
