"""Hand-built paired sets for the word edges of the redirected-mate substring
test (mate_occurs, mg_mates.hip) and for the order, dedup and count edges of
the list build, shared by tests/test_mate_edges_host.py (host mirror, CPU) and
tests/test_mate_edges.py (device).  Every set asserts its preconditions from
the plain restatement (mates_ref) and the oracle's superReadIDs, never from
the code under test, so a set that stops exercising its edge fails instead of
passing vacuously.  No native code of the product."""
import functools
import random

import numpy as np

import mates_ref as R

L_MATE = 10  # min_overlap of every set here: the shortest legal mate is 11 bp
MAX_REDRAWS = 20

# class -> container lengths: the slot width of a context is that of its longest read, so
# each class is a context of its own and its longest container fills the slot's last word
CLASSES = {
    "w1": (31, 32), "w2": (33, 63, 64), "w5": (129, 160), "w8": (225, 256), "w32": (993, 1024),
    "long": (1025, 3000), "long64k": (60000,),
}
SWEEP_L = (11, 16, 31, 32, 33, 63, 64, 65)
SWEEP_L_64K = (11, 33, 65)  # the per-thread scan over 60 kb stays short
DECOY_L = (20, 31, 32, 33, 40, 64, 65, 100)


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def changed(rng, m, p):
    """m with base p replaced by another one."""
    return m[:p] + rng.choice([c for c in "ACGT" if c != m[p]]) + m[p + 1:]


def container(rng, n, body=""):
    """n bases that are their own canonical string: 'A' first, `body` next, the
    last base not 'T' (so the other strand starts with T, G or C)."""
    fill = n - 1 - len(body)
    assert fill >= 1
    return "A" + body + rand_seq(rng, fill - 1) + rng.choice("ACG")


def sweep_offsets(n, L):
    return sorted({s for s in (0, 1, 31, 32, 33, n - L - 1, n - L) if 0 <= s <= n - L})


def near_miss_positions(L):
    """The bases a forward near-miss differs in: the last one, the first of the
    base-by-base tail, the last of the packed word, the first."""
    return sorted({p for p in (L - 1, 32, 31, 0) if p < L}, reverse=True)


def decoy_room(L):
    """The longest a decoy container's planted part can get (with its first and last base)."""
    return 1 + len(near_miss_positions(L)) * (L + 4) + L + 1


class Case:
    """One planted mate: raw record `mate` of pair `pair`, cut from strand
    `strand` ('+': the container's forward string, '-': its other strand) of
    container `cont` at offset s (sweep) or planted behind near-misses (decoy)."""

    def __init__(self, cls, kind, L, s, strand, cont, mate):
        self.cls, self.kind, self.L, self.s, self.strand, self.cont, self.mate = cls, kind, L, s, strand, cont, mate
        self.found = strand == "+"
        self.own_canonical = mate <= R.rc(mate)
        self.pair = self.side = None  # filled by the pairing

    def label(self):
        return "(%s, %s, L=%d, s=%s, %s)" % (self.cls, self.kind, self.L, self.s, self.strand)


def _sweep_container(rng, cls, n, lengths):
    F = container(rng, n)
    Rv = R.rc(F)
    cases = []
    for L in lengths:
        if L >= n:
            continue
        for s in sweep_offsets(n, L):
            cases.append(Case(cls, "sweep", L, s, "+", F, F[s:s + L]))
            cases.append(Case(cls, "sweep", L, s, "-", F, Rv[s:s + L]))
    return F, cases


def _decoy_container(rng, cls, n, L, strand, own):
    m = rand_seq(rng, L)
    if (m <= R.rc(m)) != own:
        m = R.rc(m)
    body = ""
    for p in near_miss_positions(L):
        body += changed(rng, m, p) + rand_seq(rng, rng.randrange(1, 5))
    body += m if strand == "+" else R.rc(m)
    F = container(rng, n, body)
    return F, [Case(cls, "decoy", L, None, strand, F, m)]


def _local_ok(F, cases):
    """The preconditions one container decides alone."""
    if not (R.passes(F, L_MATE) and F < R.rc(F)):
        return False
    for c in cases:
        if not R.passes(c.mate, L_MATE) or (c.mate <= R.rc(c.mate)) != c.own_canonical:
            return False
        at = F.find(c.mate)
        if c.strand == "-":
            if at != -1:
                return False
        elif at != c.s if c.kind == "sweep" else at < 0:
            return False
    return True


def oracle_super(records, l):
    """(reads in ID order, superReadID per ID) of the raw records, from the oracle."""
    from oracle import OracleDataset

    od = OracleDataset.from_strings(list(records), l)
    reads = [od.read(i) for i in range(1, od.num_unique + 1)]
    _, _, sup, _ = od.overlaps_digest(l, 4, want_super=True)
    return reads, sup.astype(np.uint32)


class MateSet:
    """One context's input: `raw` = the mates two per pair, `singles` = the
    further records of the Dataset (the containers), `reads` and `super_ids`
    from the restatement and the oracle."""

    def __init__(self, name, raw, ppd, singles, cases=(), redraws=0, l=L_MATE):
        self.name, self.raw, self.ppd, self.singles, self.l = name, list(raw), tuple(ppd), list(singles), l
        self.cases, self.redraws = list(cases), redraws
        self.records = self.singles + self.raw  # every record of the Dataset
        self.reads = R.dataset_of(self.records, l)
        oreads, self.super_ids = oracle_super(self.records, l)
        assert oreads == self.reads
        self.ids = {s: i + 1 for i, s in enumerate(self.reads)}

    def read_id(self, raw):
        return self.ids[min(raw, R.rc(raw))]

    def pair_records(self):
        """(text, offsets) of the mates, as the C-ABI takes them."""
        return R.records_of(self.raw)

    @functools.lru_cache(maxsize=None)
    def want(self, use_super):
        """(start, records, good, bad) from the restatement."""
        return R.mate_lists(self.reads, self.raw, self.ppd, self.l, self.super_ids if use_super else None)

    def first_difference(self, start, recs):
        """The first planted case whose partner's list (one record: the mate's
        container and both orientation bits) differs from the restatement's
        with the redirect, or None."""
        wstart, wrecs = self.want(True)[:2]
        for c in self.cases:
            a = self.read_id(self.raw[2 * c.pair + 1 - c.side])
            got = recs[int(start[a]):int(start[a + 1])] if a + 1 < len(start) else None
            if got is None or not np.array_equal(got, wrecs[int(wstart[a]):int(wstart[a + 1])]):
                return c.label()
        return None


def _pair_up(rng, cases, partner_len, singles):
    """One pair per planted mate with a random read of its own, the mate first or second."""
    raw = []
    for p, c in enumerate(cases):
        partner = rand_seq(rng, partner_len)
        c.pair, c.side = p, rng.randrange(2)
        raw += [c.mate, partner] if c.side == 0 else [partner, c.mate]
    first = len(cases) // 2
    return raw, (first, len(cases) - first)


def _bad_containers(s):
    """Containers of the set whose plants break a precondition only the whole
    set decides: the oracle's superReadID of a planted mate is its container,
    containers and partners are contained in nothing, every partner is a read
    of its own."""
    bad = set()
    for c in s.cases:
        if int(s.super_ids[s.read_id(c.mate)]) != s.read_id(c.cont):
            bad.add(c.cont)
        partner = s.raw[2 * c.pair + 1 - c.side]
        if s.super_ids[s.read_id(partner)] or partner in s.singles or s.raw.count(partner) != 1:
            bad.add(c.cont)
    for F in s.singles:
        if s.super_ids[s.read_id(F)]:
            bad.add(F)
    return bad


def _groups_complete(cases):
    """In each of L < 32, L = 32, L > 32: both planted strands x the raw record
    being or not being its own canonical string."""
    seen = {}
    for c in cases:
        seen.setdefault((c.L > 32) - (c.L < 32), set()).add((c.strand, c.own_canonical))
    return all(len(v) == 4 for v in seen.values()), seen


@functools.lru_cache(maxsize=None)
def class_set(cls, seed=1):
    """The sweep and decoy containers of one class with their planted mates."""
    rng = random.Random("%s/%d" % (cls, seed))
    lengths = CLASSES[cls]
    sweep_L = SWEEP_L_64K if cls == "long64k" else SWEEP_L
    makers = [functools.partial(_sweep_container, rng, cls, n, sweep_L) for n in lengths]
    for L in DECOY_L:
        fit = [n for n in lengths if n >= decoy_room(L)]
        if not fit or (cls == "long64k" and L not in SWEEP_L_64K):
            continue
        for strand in "+-":
            for own in (True, False):
                makers.append(functools.partial(_decoy_container, rng, cls, fit[0], L, strand, own))
    redraws = 0

    def draw(make):
        nonlocal redraws
        while True:
            F, cases = make()
            if _local_ok(F, cases):
                return F, cases
            redraws += 1
            assert redraws <= MAX_REDRAWS, "%s: more than %d redraws" % (cls, MAX_REDRAWS)

    drawn = [draw(m) for m in makers]
    partner_len = min(40, min(lengths))
    while True:
        conts = [F for F, _ in drawn]
        cases = [c for _, cs in drawn for c in cs]
        assert len(set(conts)) == len(conts)
        singles = [F if rng.random() < .5 else R.rc(F) for F in conts]
        raw, ppd = _pair_up(rng, cases, partner_len, singles)
        s = MateSet(cls, raw, ppd, singles, cases, redraws)
        bad = _bad_containers(s)
        complete, seen = _groups_complete(cases)
        if not bad and complete:
            break
        if not bad:  # a strand x canonical combination is missing: another first sweep container
            bad = {conts[0]}
        for k, (F, _) in enumerate(drawn):
            if F in bad:
                redraws += 1
                assert redraws <= MAX_REDRAWS, "%s: more than %d redraws (%s)" % (cls, MAX_REDRAWS, seen)
                drawn[k] = draw(makers[k])
    check_class(s)
    return s


def expected_cases(cls):
    """How many planted mates the class must hold: nothing may be left out."""
    lengths = CLASSES[cls]
    sweep_L = SWEEP_L_64K if cls == "long64k" else SWEEP_L
    n = sum(2 * len(sweep_offsets(n, L)) for n in lengths for L in sweep_L if L < n)
    for L in DECOY_L:
        if any(n >= decoy_room(L) for n in lengths) and not (cls == "long64k" and L not in SWEEP_L_64K):
            n += 4
    return n


def check_class(s):
    """Every precondition of a class set, from the restatement and the oracle."""
    assert s.redraws <= MAX_REDRAWS
    assert len(s.cases) == expected_cases(s.name) and len(s.raw) == 2 * len(s.cases)
    assert all(R.passes(r, s.l) for r in s.records)
    assert not _bad_containers(s)
    conts = {c.cont for c in s.cases}
    assert sorted(len(F) for F in conts if any(c.cont == F and c.kind == "sweep" for c in s.cases)) == \
        sorted(CLASSES[s.name])
    assert max(len(r) for r in s.reads) == max(CLASSES[s.name])
    for c in s.cases:
        F = c.cont
        assert F[0] == "A" and F[-1] != "T" and F < R.rc(F) and F in s.reads
        assert s.raw[2 * c.pair + c.side] == c.mate and len(c.mate) == c.L
        at = F.find(c.mate)
        if c.strand == "-":
            assert at == -1 and R.rc(c.mate) in F and not c.found
        elif c.kind == "sweep":
            assert at == c.s and c.found
        else:
            assert at >= 0 and c.found
        if c.kind == "decoy":  # every near-miss lies in front of the true occurrence
            true_at = F.find(c.mate if c.strand == "+" else R.rc(c.mate))
            for p in near_miss_positions(c.L):
                assert any(F[q + p] != c.mate[p] and F[q:q + p] == c.mate[:p]
                           and F[q + p + 1:q + c.L] == c.mate[p + 1:] for q in range(1, true_at)), (c.label(), p)
    complete, seen = _groups_complete(s.cases)
    assert complete, seen
    # what the redirect changes: found and not found, both on either raw strand
    want, plain = s.want(True), s.want(False)
    assert not np.array_equal(want[1], plain[1])
    assert want[2] == len(s.cases) and want[3] == 0


# ---- order and dedup
HUB_MATES, REPEATS, ALTERNATIONS = 3000, 1000, 50
N_DATASETS = 256


@functools.lru_cache(maxsize=None)
def order_set():
    """One context of 50-bp reads, 256 datasets of which 0, 3 and 255 hold
    pairs: a hub read with 3,000 distinct mates in input order, one pair
    repeated 1,000 times, a pair alternating between two orientations, the same
    pair in datasets 3 and 255 on every strand choice, a read paired with
    itself on both strands, and a bad pair in the middle."""
    rng = random.Random("order/1")

    def canon():
        x = rand_seq(rng, 50)
        return min(x, R.rc(x))

    hub, a, b, x, e, f = (canon() for _ in range(6))
    d0 = []
    for k in range(HUB_MATES):
        h, m = (hub, R.rc(hub))[(k >> 1) & 1], canon()
        m = R.rc(m) if k % 3 == 0 else m
        d0 += [h, m] if k % 2 == 0 else [m, h]
        if k == HUB_MATES // 2:
            d0 += [e, "ACGTNACGTACGTACGTACGT"]  # a bad pair in the middle
    d0 += [e, f] * REPEATS
    for k in range(ALTERNATIONS):
        d0 += [a, b if k % 2 == 0 else R.rc(b)]
    d0 += [x, x, x, R.rc(x)]
    four = [a, b, a, R.rc(b), R.rc(a), b, R.rc(a), R.rc(b)]  # orient 3, 2, 1, 0
    ppd = [0] * N_DATASETS
    ppd[0], ppd[3], ppd[255] = len(d0) // 2, 4, 4
    s = MateSet("order", d0 + four + four, ppd, [])
    # ---- that it holds its cases, from the restatement
    assert not s.super_ids.any()
    start, recs, good, bad = s.want(False)
    assert bad == 1 and good == len(s.raw) // 2 - 1 and len(recs) < 2 * good

    def lst(read):
        i = s.read_id(read)
        return recs[int(start[i]):int(start[i + 1])]

    h = lst(hub)
    assert len(h) == HUB_MATES and len(set(h["id"].tolist())) == HUB_MATES
    assert np.any(np.diff(h["id"].astype(np.int64)) < 0), "the hub's list is in ID order: input order is not tested"
    assert set(h["orient"].tolist()) == {0, 1, 2, 3}
    assert len(lst(e)) == 1 and len(lst(f)) == 1  # 1,000 equal records each, one kept
    la = lst(a)
    assert [(int(r["orient"]), int(r["dataset"])) for r in la] == \
        [(3, 0), (2, 0), (3, 3), (2, 3), (1, 3), (0, 3), (3, 255), (2, 255), (1, 255), (0, 255)]
    assert [(int(r["id"]), int(r["orient"])) for r in lst(x)] == [(s.read_id(x), o) for o in (3, 2, 1)]
    assert set(np.unique(recs["dataset"]).tolist()) == {0, 3, 255}
    assert np.any((recs["dataset"] == 255) & (recs["orient"] == 3))  # sort key 1023
    return s


# ---- count edges
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def count_pool():
    """257 pairs of 50-bp reads, every fifth one bad; the Dataset holds all of them."""
    rng = random.Random("count/1")
    raw = []
    for p in range(max(COUNTS)):
        a, b = rand_seq(rng, 50), rand_seq(rng, 50)
        if p % 5 == 4:
            b = b[:20] + "N" + b[21:]
        raw += [a, b]
    s = MateSet("counts", raw, (len(raw) // 2,), [])
    assert s.want(False)[2:] == (max(COUNTS) - max(COUNTS) // 5, max(COUNTS) // 5)
    return s


def count_want(n_pairs):
    """(raw, ppd, (start, records, good, bad)) of the pool's first n_pairs pairs."""
    s = count_pool()
    raw = s.raw[:2 * n_pairs]
    return raw, (n_pairs,), R.mate_lists(s.reads, raw, (n_pairs,), s.l, None)
