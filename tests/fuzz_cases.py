"""Long random operation sequences on dense keys for the resident trie and forest: the generator
and the model of tests/test_gpu_commit_fuzz.py (device) and tests/test_commit_fuzz_model.py (the
model alone, on the CPU).  No GPU, no torch; the oracle module is handed in.

Dense keys.  Per seed: a base key of 64 nibbles, a set P of split positions (EDGE, the depths at
and around the 16-nibble words of forest.h's prefix_word, plus four random ones) and per position
an alphabet of three nibbles.  Every key equals the base outside P, so a branch can only sit at a
depth of P and every extension length is a gap of P.

The model is oracle.Trie plus the log of accepted batches.  The oracle has no copy and no
rollback, and a batch it refuses leaves it half-updated: each of these is a fresh oracle.Trie with
the log replayed up to the wanted point.  Expected roots never come from a key -> value dict:
khipu's value-only branch (forest.h VB_DEPTH) makes the trie depend on its history.

One rule keeps a batch inside the engine's batch contract ("Repeated puts": one op per
key, the last one wins, upserts before deletes).  The reference's fold of a batch depends on the
order of the puts INSIDE it only where a put meets a leaf with no path left, so a batch here never
holds two different upsert keys that share 63 nibbles, nor a second op on a key that has a live
63-nibble sibling.  Across batches every such shape is kept: that is how value-only branches are
made, updated and refused.

The step list is a pure function of the seed and the model's answers: replay(seed, upto) gives it
again as data.
"""
import random

from khipu_amd import codec
from tests import partial_cases as P
from tests import writeback as W

EDGE = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63]
TRIE_SEEDS = [101, 103, 104, 110, 111, 112, 113, 116, 117, 119, 123, 125]
FOREST_SEEDS = [201, 202, 203, 204, 205, 206]
FOREST_IDS = [0, 7, 4999, 65535, 70000]  # 0 and the largest id of test_forest_trie_id_bits
NSTEPS = 60
TRIE_OPS = ("savepoint", "rollback", "release", "root_of", "copy", "compact", "export", "partial", "fill_all", "prove")
FOREST_OPS = ("savepoint", "rollback", "release", "compact", "prove", "evict", "load", "load_partial")


def nibbles(key):
    return [x for b in key for x in (b >> 4, b & 15)]


def from_nibbles(n):
    return bytes((n[2 * i] << 4) | n[2 * i + 1] for i in range(32))


def lcp(a, b):
    """Common prefix of two 32-byte keys in nibbles."""
    x = int.from_bytes(a, "big") ^ int.from_bytes(b, "big")
    return 64 if not x else (256 - x.bit_length()) // 4


def siblings63(live, k):
    """The keys of `live` that share exactly 63 nibbles with k."""
    return [x for x in (k[:31] + bytes([(k[31] & 0xF0) | n]) for n in range(16)) if x != k and x in live]


class Keys:
    def __init__(self, r):
        self.base = [r.randrange(16) for _ in range(64)]
        self.P = sorted(EDGE + r.sample([p for p in range(2, 62) if p not in EDGE], 4))
        self.alpha = {p: [self.base[p]] + r.sample([x for x in range(16) if x != self.base[p]], 2) for p in self.P}

    def key(self, r):
        n = list(self.base)
        for p in self.P:
            if r.random() >= 0.6:
                n[p] = r.choice(self.alpha[p][1:])
        return from_nibbles(n)

    def sibling(self, r, k):
        n = nibbles(k)
        p = r.choice(self.P)
        n[p] = r.choice([x for x in self.alpha[p] if x != n[p]])
        return from_nibbles(n)


def value(r):
    """A value from a pool that straddles the engine's size rules (inline / hashed nodes, the RLP
    55/56 and 255/256 length forms, one byte below and at 0x80)."""
    kind = r.randrange(17)
    if kind == 0:
        return bytes([r.randrange(1, 0x80)])
    if kind == 1:
        return bytes([r.randrange(0x80, 0x100)])
    if kind < 14:
        n = [2, 20, 29, 30, 31, 32, 33, 34, 55, 56, 255, 256][kind - 2]
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 14:
        return codec.account_rlp(r.randrange(1 << 16), r.randrange(10 ** 22))
    return codec.storage_value_rlp(r.choice([1, 0x7F, 0x80, r.randrange(2 ** 255, 2 ** 256)]))


class Model:
    """oracle.Trie plus the log of accepted batches.  `live` (key -> value) is book-keeping for the
    generator and for len(); `store` is every node reachable at a settled version since the model
    was built, the node store a write-back contract is checked against."""

    def __init__(self, O, log=()):
        self.O = O
        self.log = list(log)
        self.t = O.Trie()
        self.live, self.vb = {}, set()
        for ups, dels in self.log:
            self.live, self.vb = self._fold(self.t, self.live, self.vb, ups, dels)
        self.t.persist().reopen()
        self.store = dict(W.reachable(self.t))
        self.pending = False

    @staticmethod
    def _fold(t, live, vb, ups, dels):
        live, vb = dict(live), set(vb)
        for k, v in ups:
            t.put(k, v)
            if k in live and siblings63(live, k):
                vb.add(k)  # (a put into a leaf with no path left: khipu's value-only branch; book-keeping only)
            live[k] = v
        for k in dels:
            t.remove(k)
            live.pop(k, None)
            vb.discard(k)
        return live, vb

    def settle(self):
        """The last accepted batch's nodes join the store and the oracle's Updated log starts empty."""
        if self.pending:
            self.store.update(W.reachable(self.t))
            self.t.persist().reopen()
            self.pending = False

    def commit(self, ups, dels):
        """True: accepted, the Updated log left open for writeback.check_delta (settle() closes it).
        False: the oracle raised -- an expected refusal; the model is the version before the batch."""
        self.settle()
        try:
            self.live, self.vb = self._fold(self.t, self.live, self.vb, ups, dels)
        except self.O.OracleError:
            self.__init__(self.O, self.log)
            return False
        self.log.append((list(ups), list(dels)))
        self.pending = True
        return True

    def fork(self, upto=None):
        return Model(self.O, self.log if upto is None else self.log[:upto])

    def root_of(self, ups, dels):
        m = self.fork()
        return m.root() if m.commit(ups, dels) else None

    def root(self):
        return self.t.root_hash()

    def __len__(self):
        return len(self.live)

    def nodes(self):
        return W.reachable(self.t)

    def has_sibling63(self, k):
        return bool(siblings63(self.live, k))


def make_batch(r, K, m, shy, nu=None, nd=None):
    """(upserts, deletes, made a value-only branch) over model m.  shy: keys whose delete was refused."""
    nu = r.choice([0, 1, 3, 12, 40]) if nu is None else nu
    nd = r.choice([0, 0, 1, 4, 16]) if nd is None else nd
    live = sorted(m.live)
    deep = [k for a, b in zip(live, live[1:]) if lcp(a, b) == 63 for k in (a, b)]  # (a re-put of one makes a value-only branch)
    ups, dels = [], []
    for _ in range(nu):
        x = r.random()
        if deep and x < 0.06:
            k = r.choice(deep)
        elif live and x < 0.3:
            k = r.choice(live)
        elif live and x < 0.65:
            k = K.sibling(r, r.choice(live))
        else:
            k = K.key(r)
        ups.append((k, value(r)))
    for _ in range(nd):
        if live and r.random() < 0.8:
            k = r.choice(live)
            if k in shy and r.random() < 0.95:
                k = r.choice(live)
        else:
            k = K.sibling(r, r.choice(live)) if live and r.random() < 0.5 else K.key(r)
        dels.append(k)
    # the rule of the module's docstring
    first = {}
    for k, _ in ups:
        first.setdefault(k[:31] + bytes([k[31] & 0xF0]), k)
    ups = [(k, v) for k, v in ups if first[k[:31] + bytes([k[31] & 0xF0])] == k]
    seen, out = set(), []
    for k, v in reversed(ups):
        if k in seen and m.has_sibling63(k):
            continue
        seen.add(k)
        out.append((k, v))
    ups = out[::-1]
    dels = [k for k in dels if not (k in seen and m.has_sibling63(k))]
    vb = sorted({k for k, _ in ups if k in m.live and m.has_sibling63(k)})
    return ups, dels, vb


def path_set(nodes, root, keys):
    out = set()
    if root != W.EMPTY_TRIE_HASH:
        for k in keys:
            out.update(P.path_hashes(nodes, root, k)[0])
    return out


def probe(r, K, m, dead):
    live = sorted(m.live)
    q = r.sample(live, min(12, len(live))) + r.sample(dead, min(6, len(dead))) + [K.key(r) for _ in range(3)]
    if live:
        q.append(K.sibling(r, r.choice(live)))
    return q


def _pick(r, weights, counts):
    """An operation kind among those valid now; every other time one that has run less than twice."""
    kinds = sorted(weights)
    need = [k for k in kinds if k != "commit" and counts.get(k, 0) < 2]
    if need and r.random() < 0.5:
        return r.choice(need)
    return r.choices(kinds, [weights[k] for k in kinds])[0]


def trie_run(seed, O, nsteps=NSTEPS):
    """Yields (index, step, model) after the model took the step.  step is plain data: "op" and its
    arguments, "probe" (keys for get), and what the model answers: "refused", "root", "len".
    Partial handles: "held" is the set of node hashes the handle is known to hold (None: all)."""
    r = random.Random(seed)
    K = Keys(r)
    n0 = r.choice([0, 1, 40, 200])
    init = {}
    while len(init) < n0:
        k = K.key(r) if not init or r.random() < 0.5 else K.sibling(r, r.choice(sorted(init)))
        if not any(lcp(k, x) == 63 for x in init):  # (a batch build: the canonical trie, no put order to follow)
            init[k] = value(r)
    m = Model(O, [(list(init.items()), [])])
    shy, dead, saves, counts = set(), [], [], {}
    wb = None  # the write-back bounds of the last accepted commit (must be emitted, may be emitted), if known
    held, safe = None, set()  # a partial handle: (an upper bound of) the node hashes it holds, the keys it has put
    forced = None
    ncopy = 0
    step = dict(op="open", ups=list(init.items()), probe=probe(r, K, m, dead), root=m.root(), len=len(m), depth=0)
    yield 0, step, m
    for i in range(1, nsteps + 1):
        m.settle()
        depth = len(saves)
        w = dict(commit=30, root_of=4, copy=4, compact=4, prove=4)
        if depth < 3:
            w["savepoint"] = 6
        if depth:
            w["rollback"], w["release"] = 6, 5
        else:
            w["export"] = 3
            if m.live:
                w["partial"] = 3
            if held is not None:
                w["fill_all"] = 2
        op = "commit" if forced else _pick(r, w, counts)
        if op == "export" and held is not None:
            op = "fill_all"  # (an export of the whole trie needs the whole trie)
        counts[op] = counts.get(op, 0) + 1
        step = dict(op=op)
        if op in ("commit", "root_of"):
            ups, dels, vb = forced or make_batch(r, K, m, shy)
            forced = None
            tempt = sorted(k for k in m.vb if k not in {u for u, _ in ups})
            if tempt and depth and held is None and r.random() < 0.3:
                dels = dels + [r.choice(tempt)]  # the delete of a value-only branch's key: a refusal under a savepoint
            if held is not None and depth:
                # no fill under a savepoint: only new values for keys this handle has put (their paths are held)
                ups = [(k, v) for k, v in ups if k in safe and k in m.live]
                if not ups:
                    ups = [(k, value(r)) for k in r.sample(sorted(safe & set(m.live)), min(3, len(safe & set(m.live))))]
                dels = []
                vb = sorted({k for k, _ in ups if m.has_sibling63(k)})
            step.update(ups=ups, dels=dels, vb=vb)
            keys = [k for k, _ in ups] + dels
            if held is not None:
                # held is an upper bound of what the handle holds: a path node outside it must be fetched,
                # and everything the reference's walk and fix may load counts as held afterwards
                step["must_fetch"] = not path_set(m.store, m.root(), keys) <= held
                step["allowed"] = P.fetchable(m.store, m.root(), keys)
                if not depth:
                    held = held | step["allowed"]
            if op == "root_of":
                step["want"] = m.root_of(ups, dels)
            else:
                before = set(m.live)
                step["refused"] = not m.commit(ups, dels)
                wb = None
                if step["refused"]:
                    shy.update([k for k in dels if k in m.vb] or dels)
                else:
                    new, upd = m.nodes(), m.t.updated()
                    wb = ({h: e for h, e in new.items() if h not in m.store}, {h: e for h, e in new.items() if upd.get(h) == e})
                    dead = (dead + sorted(before - set(m.live)))[-40:]
                    safe = (safe | {k for k, _ in ups}) - set(dels)
                    if held is not None:
                        held = {h for h in new if h in held or h in upd}
        elif op == "savepoint":
            saves.append((len(m.log), None if held is None else set(held), set(safe), wb))
        elif op == "rollback":
            n, held, safe, wb = saves.pop()
            m = m.fork(n)
            step["wb"] = wb
        elif op == "release":
            saves.pop()
        elif op == "copy":
            ncopy += 1
            step["mode"] = "both" if ncopy % 3 == 0 else r.choice(["switch", "stay"])
            if step["mode"] == "switch":
                saves, wb = [], None  # (a copy holds the current version and no savepoints)
            if step["mode"] == "both":
                side = m.fork()
                ups, dels, _ = make_batch(r, K, side, shy, nu=3, nd=1)
                step.update(ups=ups, dels=dels, side_refused=not side.commit(ups, dels), side_root=side.root(),
                            side_len=len(side), side_probe=probe(r, K, side, dead),
                            allowed=P.fetchable(m.store, m.root(), [k for k, _ in ups] + dels))
                side.settle()
                step["side"] = side
        elif op == "compact":
            step["refused"] = depth > 0
            wb = wb if depth else None
        elif op == "export":
            step["want"] = m.nodes()
            wb = None
        elif op == "partial":
            forced = make_batch(r, K, m, shy, nu=r.choice([3, 12]), nd=r.choice([1, 4]))
            keys = [k for k, _ in forced[0]] + forced[1]
            some = r.sample(keys, len(keys) // 2) + r.sample(sorted(m.live), min(3, len(m.live)))
            wit = path_set(m.store, m.root(), some) | {m.root()}
            step["witness"] = {h: m.store[h] for h in sorted(wit)}
            held, safe, wb = P.held(step["witness"], m.root())[0], set(), None
        elif op == "fill_all":
            held, wb = None, None
        elif op == "prove":
            step["keys"] = probe(r, K, m, dead)
        step.update(probe=probe(r, K, m, dead), root=m.root(), len=len(m), depth=len(saves),
                    held=None if held is None else set(held), safe=set(safe) if held is not None else set())
        yield i, step, m


def replay(seed, upto, O=None):
    """The first `upto` steps of trie sequence `seed` as data (the models dropped)."""
    if O is None:
        from oracle import oracle as O
    out = []
    for i, step, _ in trie_run(seed, O):
        out.append({k: v for k, v in step.items() if k != "side"})
        if i + 1 >= upto:
            break
    return out


def forest_run(seed, O, nsteps=NSTEPS):
    """Yields (index, step, models, resident) for a forest of FOREST_IDS: models {id: Model},
    resident the ids the forest holds.  One key generator serves every trie, so equal keys meet."""
    r = random.Random(seed)
    K = Keys(r)
    ms = {t: Model(O) for t in FOREST_IDS}
    resident = set(FOREST_IDS)
    shy, saves, counts = set(), [], {}
    yield 0, dict(op="open", probe=[], depth=0), ms, resident
    for i in range(1, nsteps + 1):
        for m in ms.values():
            m.settle()
        depth = len(saves)
        evicted = sorted(set(FOREST_IDS) - resident)
        w = dict(commit=30, compact=4, prove=4)
        if depth < 3:
            w["savepoint"] = 4
        if depth:
            w["rollback"], w["release"] = 4, 3
        elif resident and i > 8:
            w["evict"] = 5
        if evicted:
            w["load"] = 6
            if not depth and any(ms[t].live for t in evicted):
                w["load_partial"] = 5
        op = _pick(r, w, counts)
        counts[op] = counts.get(op, 0) + 1
        step = dict(op=op)
        if op == "commit":
            ups, dels, touched = [], [], []
            for t in r.sample(sorted(resident), min(len(resident), r.choice([1, 2, 3, 5]))):
                m = ms[t]
                if m.live and r.random() < 0.15:  # to empty (and back, by a later batch)
                    u, d = [], [k for k in sorted(m.live) if k not in m.vb or r.random() < 0.02]
                else:
                    u, d, _ = make_batch(r, K, m, shy, nu=r.choice([1, 3, 12, 40]))
                ups += [(t, k, v) for k, v in u]
                dels += [(t, k) for k in d]
                if u or d:
                    touched.append(t)
            logs = {t: len(ms[t].log) for t in touched}
            ok = [ms[t].commit([(k, v) for x, k, v in ups if x == t], [k for x, k in dels if x == t]) for t in touched]
            step["refused"] = not all(ok)
            if step["refused"]:  # all or nothing
                shy.update([k for t, k in dels if k in ms[t].vb] or [k for _, k in dels])
                for t in touched:
                    ms[t] = ms[t].fork(logs[t])
            step.update(ups=ups, dels=dels, touched=touched)
        elif op == "savepoint":
            saves.append(({t: len(m.log) for t, m in ms.items()}, set(resident)))
        elif op == "rollback":
            logs, resident = saves.pop()
            ms = {t: m.fork(logs[t]) if len(m.log) != logs[t] else m for t, m in ms.items()}
        elif op == "release":
            saves.pop()
        elif op == "compact":
            step["refused"] = depth > 0
        elif op == "evict":
            step["ids"] = r.sample(sorted(resident), r.randrange(1, len(resident) + 1))
            resident -= set(step["ids"])
        elif op == "load":
            step["ids"] = r.sample(evicted, r.randrange(1, len(evicted) + 1))
            resident |= set(step["ids"])
        elif op == "load_partial":
            t = r.choice([t for t in evicted if ms[t].live])
            m = ms[t]
            some = r.sample(sorted(m.live), min(len(m.live), r.choice([1, 4])))
            wit = path_set(m.store, m.root(), some) | {m.root()}
            step.update(id=t, witness={h: m.store[h] for h in sorted(wit)},
                        held=P.held({h: m.store[h] for h in wit}, m.root())[0])
            resident.add(t)
        q = []
        for t in FOREST_IDS:
            live = sorted(ms[t].live)
            q += [(t, k) for k in r.sample(live, min(4, len(live)))] + [(t, K.key(r))]
            others = sorted(k for x in FOREST_IDS if x != t for k in ms[x].live if k not in ms[t].live)
            q += [(t, k) for k in r.sample(others, min(2, len(others)))]  # another trie's key
        step.update(probe=q, depth=len(saves))
        yield i, step, ms, resident
