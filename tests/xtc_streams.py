"""Hand-built XTC frame records with known integers -- the data of
tests/test_xtc_streams.py (CPU tier) and tests/test_gpu_xtc_streams.py (GPU
tier).  Not a test module, and it never calls the product.

``build_frame`` is a plain-Python encoder of one compressed frame record from
an explicit list of groups.  It restates the decoder of oracle/xtc_py.py the
other way round:

  * a packed triple is ``(v0*s1 + v1)*s2 + v2`` in ``nbits`` bits, its full
    bytes least significant first (8 bits each), then the top 1..8 bits;
    ``nbits`` is the bit length of ``s0*s1*s2`` for the large triple and the
    small-integer index for a small one (sizes magicints[index], 3 times);
  * when any axis range ``maxint - minint + 1`` exceeds 0xffffff the large
    triple is three raw fields of each range's bit length instead;
  * a group is one large triple, a flag bit, a 5-bit code ``3*n_small +
    is_smaller + 1`` (<= 31) when the flag is set, and ``n_small`` small
    triples of the index in force *before* ``is_smaller`` is applied.  The
    flag is written when the run or the index changes (or on request);
  * with a run, the first small triple is atom i, relative to the large one
    (which is atom i+1: the writer's water swap); the second is relative to
    atom i, the others are chained.  Relative means ``+ t - magicints[idx]//2``.

So the reference of a built stream is the integers that went into it:
``Frame.ints`` and ``expected_angstrom``.  ``Frame.layout`` records where every
group lies, so that a test can assert what a stream reaches (a width inside a
run, a word boundary straddled, a stretch of clean groups, a batch position).

The zoo (``VALID``, ``BROKEN``, ``stream(name)``, ``check_reach(name)``) names
the streams and what each is for; see DESIGN.md, "XTC decompressed on the
GPU".  Device terms used below: the wave keeps kRing = 4096 stream words in an
LDS ring, filled in stages of 512; it records groups in batches of 64 (group
number % 64 is the lane) and decodes a batch when it is full; the scan of
flag-free ("clean") groups looks at most 192 words ahead.
"""
import collections
import functools
import random
import struct

import numpy as np

MAGICINTS = [0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322,
             406, 512, 645, 812, 1024, 1290, 1625, 2048, 2580, 3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384,
             20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072, 165140, 208063, 262144, 330280,
             416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304,
             5284491, 6658042, 8388607, 10568983, 13316085, 16777216]
FIRSTIDX, LASTIDX = 9, 72
I32_MIN, I32_MAX = -2**31, 2**31 - 1
RING_WORDS, STAGE_WORDS, BATCH, SCAN_WORDS = 4096, 512, 64, 192

Group = collections.namedtuple("Group", "bit atom idx nsmall flagged nbits")
Frame = collections.namedtuple(
    "Frame", "record ints layout n_atoms declared precision large_bits packed stream_bits nbytes n_words")


class _Bits:
    """MSB-first bit writer; whole bytes leave the accumulator every 2048 bits."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0
        self.total = 0

    def put(self, v, n):
        assert 0 <= v < (1 << n), (v, n)
        self.acc = (self.acc << n) | v
        self.n += n
        self.total += n
        if self.n >= 2048:
            r = self.n & 7
            self.buf += (self.acc >> r).to_bytes(self.n >> 3, "big")
            self.acc &= (1 << r) - 1
            self.n = r

    def put_packed(self, vals, sizes, nbits):
        val = (vals[0] * sizes[1] + vals[1]) * sizes[2] + vals[2]
        assert val < (1 << nbits), (vals, sizes, nbits)
        q, r = divmod(nbits, 8)
        if r == 0 and q > 0:
            q, r = q - 1, 8
        for k in range(q):
            self.put((val >> (8 * k)) & 0xFF, 8)
        if r:
            self.put(val >> (8 * q), r)

    def bytes(self):
        pad = -self.n % 8
        acc, n = self.acc << pad, self.n + pad
        return bytes(self.buf) + (acc.to_bytes(n >> 3, "big") if n else b"")


class Values:
    """Seeded source of triples in [0, s): about a tenth all zero and a tenth
    all s - 1; in the rest each axis is 0 or s - 1 with probability 0.15 each
    and uniform otherwise.  A packed value whose last field is 0 is an exact
    multiple of its divisor: there the quotient estimate d * (1/s) of the
    double-precision split can round below the quotient, which is the case
    its one-step correction exists for (all-zero triples alone never show it:
    their quotient is 0)."""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def _axis(self, s):
        u = self.r.random()
        return 0 if u < 0.15 else s - 1 if u < 0.3 else self.r.randrange(s)

    def triple(self, sizes):
        u = self.r.random()
        if u < 0.1:
            return [0, 0, 0]
        if u < 0.2:
            return [s - 1 for s in sizes]
        return [self._axis(s) for s in sizes]


def build_frame(minint, maxint, smallidx, precision, groups, values, flag_all=False, declared_natoms=None,
                nbytes_delta=0, _unchecked=False):
    """One XTC frame record.  ``groups``: (n_small in 0..10, is_smaller in
    -1/0/+1[, force the flag]) each.  ``declared_natoms``: the atom count the
    headers announce (default: what the groups hold).  ``nbytes_delta``: added
    to the stream's byte count in the header, the stream cut to match.
    ``_unchecked``: run_at_index_8() only."""
    sizeint = [maxint[c] - minint[c] + 1 for c in range(3)]
    assert all(0 < s < 2**32 for s in sizeint)
    per_axis = max(sizeint) > 0xFFFFFF
    axis_bits = [s.bit_length() for s in sizeint]
    large_bits = sum(axis_bits) if per_axis else (sizeint[0] * sizeint[1] * sizeint[2]).bit_length()
    if not (FIRSTIDX <= smallidx <= LASTIDX):
        raise ValueError("start index outside the table")
    w = _Bits()
    atoms, layout = [], []
    run, idx, stepped_out = 0, smallidx, False
    for g in groups:
        n_small, is_smaller, force = g[0], g[1], len(g) > 2 and g[2]
        if stepped_out:
            raise ValueError("a group after the index left the table")
        code = 3 * n_small + is_smaller + 1
        if not (0 <= n_small <= 10 and is_smaller in (-1, 0, 1) and code <= 31):
            raise ValueError(f"group {g} has no run code")
        if n_small > 0 and MAGICINTS[idx] == 0 and not _unchecked:
            raise ValueError("a run at index 8")
        bit = w.total
        large = values.triple(sizeint)
        if per_axis:
            for c in range(3):
                w.put(large[c], axis_bits[c])
        else:
            w.put_packed(large, sizeint, large_bits)
        flagged = flag_all or force or 3 * n_small != run or is_smaller != 0
        if flagged:
            w.put(1, 1)
            w.put(code, 5)
            run = 3 * n_small
        else:
            w.put(0, 1)
        big = [large[c] + minint[c] for c in range(3)]
        if n_small == 0:
            atoms.append(big)
        else:
            m = MAGICINTS[idx]
            half, prev = m // 2, big
            for k in range(n_small):
                t = values.triple([m] * 3) if m else [0, 0, 0]
                if m:
                    w.put_packed(t, [m] * 3, idx)
                else:
                    w.put(0, idx)
                a = [prev[c] + t[c] - half for c in range(3)]
                if k == 0:
                    atoms.append(a)
                    atoms.append(big)
                else:
                    atoms.append(a)
                prev = a
        layout.append(Group(bit, len(atoms) - 1 - n_small, idx, n_small, flagged, w.total - bit))
        idx += is_smaller
        if not (FIRSTIDX - 1 <= idx <= LASTIDX):
            stepped_out = True  # the decoders reject the stream here
    n_atoms = len(atoms)
    declared = n_atoms if declared_natoms is None else declared_natoms
    if n_atoms < 10 or declared < 10:
        raise ValueError("frames of fewer than 10 atoms are stored raw")
    if min(map(min, atoms)) < I32_MIN or max(map(max, atoms)) > I32_MAX:
        raise ValueError("an atom outside int32 (it would wrap in C; not a decoder finding)")
    ints = np.array(atoms, dtype=np.int64)
    ints.setflags(write=False)
    stream = w.bytes()
    assert len(stream) == (w.total + 7) // 8
    nbytes = len(stream) + nbytes_delta
    assert nbytes > 0
    stream = stream[:nbytes] + b"\0" * (-nbytes % 4)
    head = struct.pack(">iiif", 1995, declared, 0, 0.0) + struct.pack(">9f", 50, 0, 0, 0, 50, 0, 0, 0, 50)
    head += struct.pack(">i", declared)
    assert len(head) == 56
    comp = struct.pack(">f3i3iii", precision, *minint, *maxint, smallidx, nbytes)
    record = head + comp + stream
    assert len(record) % 4 == 0
    return Frame(record, ints, tuple(layout), n_atoms, declared, float(np.float32(precision)), large_bits,
                 not per_axis, w.total, nbytes, len(stream) // 4)


def run_at_index_8(minint, maxint, precision, values, lead):
    """The one deliberately invalid group stream: ``lead`` (valid groups from
    start index 10), two run-free steps down to index 8, then a group that
    announces a run of 2 there.  magicints[8] is 0, so its small triples have
    no values; 8 zero bits each stand in for them."""
    groups = list(lead) + [(0, -1), (0, -1), (2, 0)]
    return build_frame(minint, maxint, 10, precision, groups, values, _unchecked=True)


def expected_angstrom(ints, precision):
    """f32(f32(f32(i) * f32(1 / f64(precision))) * 10): the reader's rounding."""
    inv = np.float32(1.0 / np.float64(np.float32(precision)))
    nm = (np.asarray(ints).astype(np.float32) * inv).astype(np.float32)
    out = (nm * np.float32(10.0)).astype(np.float32)
    out.setflags(write=False)
    return out


def words_of(frame):
    """(uint32 words as the file holds them, rec_off, rec_len) of one record."""
    w = np.frombuffer(frame.record, dtype=np.uint32).copy()
    return w, np.zeros(1, dtype=np.int64), np.array([len(w)], dtype=np.int64)


# -- what a layout reaches -----------------------------------------------------------

def straddles(frame, word):
    """A group that starts before stream word ``word`` and ends inside or after it."""
    b = 32 * word
    return any(g.bit < b < g.bit + g.nbits for g in frame.layout)


def clean_stretches(frame):
    """Lengths of the maximal stretches of consecutive flag-free groups."""
    out, n = [], 0
    for g in frame.layout:
        if g.flagged:
            if n:
                out.append(n)
            n = 0
        else:
            n += 1
    if n:
        out.append(n)
    return out


def run_widths(frame):
    """Small-triple widths (indices) that occur inside runs."""
    return {g.idx for g in frame.layout if g.nsmall > 0}


def isolated_flags(frame):
    """Flagged groups with a clean group on either side."""
    L = frame.layout
    return sum(1 for k in range(1, len(L) - 1) if L[k].flagged and not L[k - 1].flagged and not L[k + 1].flagged)


# -- headers ---------------------------------------------------------------------------

def _hdr(minint, sizes):
    return tuple(minint), tuple(minint[c] + sizes[c] - 1 for c in range(3))


MARGIN = 100_000_000  # > 10 chained small offsets of magicints[72]/2: atoms stay inside int32
WIDE32 = 2**32 - 2 * MARGIN  # a 32-bit axis range that leaves that margin at both ends of int32
HEADERS = {
    "w1": _hdr((17, -5, 1000), (1, 1, 1)),                                   # packed, 1 bit (always 0)
    "w2": _hdr((-3, 40, 7), (1, 3, 1)),                                      # packed, 2 bits
    "w31": _hdr((-600, -700, 100), (1290, 1290, 1290)),                      # packed, 31 bits
    "w32": _hdr((-800, 0, -1625), (1625, 1625, 1625)),                       # packed, 32 bits
    "w38": _hdr((-2500, -3000, 0), (5000, 6000, 7000)),                      # packed, 38 bits (moderate)
    "w52": _hdr((-65000, -70000, -100000), (131071, 140001, 200003)),        # packed, exactly 52 bits: split_f64
    "w53": _hdr((-65000, -70000, -100000), (131071, 140001, 300007)),        # packed, exactly 53 bits: byte division
    "w72": _hdr((-8000000, -8388000, -1234567), (0xFFFFFF,) * 3),            # packed, 72 bits
    "a25": _hdr((-2**23, -5, -2**24), (2**24,) * 3),                         # per axis 25/25/25
    "a32x": _hdr((I32_MIN + MARGIN, -2500, -35000), (WIDE32, 5000, 70000)),  # per axis 32/13/17
    "a32_32_31": _hdr((I32_MIN + MARGIN, I32_MIN + MARGIN, -2**30 + 5), (WIDE32, WIDE32, 2**31 - 9)),
    "a96": _hdr((I32_MIN + MARGIN,) * 3, (WIDE32,) * 3),                     # per axis 32/32/32
}
LARGE_BITS = {"w1": 1, "w2": 2, "w31": 31, "w32": 32, "w38": 38, "w52": 52, "w53": 53, "w72": 72, "a25": 75,
              "a32x": 62, "a32_32_31": 95, "a96": 96}


def _frame(header, smallidx, groups, seed, precision=1000.0, **kw):
    lo, hi = HEADERS[header]
    f = build_frame(lo, hi, smallidx, precision, groups, Values(seed), **kw)
    assert f.large_bits == LARGE_BITS[header] and f.packed == header.startswith("w")
    return f


# -- group lists ------------------------------------------------------------------------

def index_walk_groups():
    """Index 9 -> 72; at each, three groups of one run length (the first sets
    it, two clean ones follow), then one that raises the index.  Run lengths
    cycle 1..10 (10 small triples and a raise have no run code: 9 there)."""
    g = []
    for idx in range(FIRSTIDX, LASTIDX + 1):
        r = 1 + (idx - FIRSTIDX) % 10
        g += [(r, 0)] * 3
        if idx < LASTIDX:
            g.append((min(r, 9), 1))
    return g


def random_groups(seed, n, start, lo, hi, p_run=0.25, p_step=0.1):
    """n groups: the run length is redrawn (0..10) with probability p_run and
    the index steps by +-1 with probability p_step, kept inside lo..hi."""
    r = random.Random(seed)
    g, run, idx = [], 0, start
    for _ in range(n):
        if r.random() < p_run:
            run = r.randrange(11)
        step = 0
        if r.random() < p_step:
            step = r.choice((-1, 1))
            if not (lo <= idx + step <= hi) or (run == 10 and step == 1):
                step = 0
        g.append((run, step))
        idx += step
    return g


def _clean_c_groups(c, n_small):
    # two flagged groups, so that the scan starts on a batch that already holds
    # records (take = min(K - done, 64 - n) with n = 2) and the middle flag is at
    # batch position (c + 2) % 64 != 0
    return [(n_small, 0, True)] * 2 + [(n_small, 0)] * c + [(n_small, 0, True)] + [(n_small, 0)] * c


def _idle_at_8_groups():
    return ([(2, 0), (2, -1), (1, 0), (0, -1)] + [(0, 0)] * 70 + [(0, 0, True)] + [(0, 0)] * 5 +
            [(0, 1), (3, 0), (3, 0), (0, 1), (4, 0)])


RUNS_0_TO_10 = [(r, 0) for r in range(11)]  # 66 atoms; every position of every run length
WORD_PER_ATOM = (511, 512, 513, 4095, 4096, 4097, 4607, 4608, 4609, 8193)
CLEAN_C = (63, 64, 65, 129)
EDGE_HEADERS = ("w2", "w52", "w53", "w72", "a25", "a32_32_31")
WALK_HEADERS = ("w1", "w72", "a32x")
WALK_PRECISIONS = {"p100": 100.0, "p10000": 10000.0, "p1234_5": 1234.5}
MIXED_N = 3200
LONG_WORDS = RING_WORDS + STAGE_WORDS  # a defect behind this word: batches written, the ring wrapped


def _lead(long):
    """Valid groups in front of a defect: a few, or enough to pass word 4608
    (38-bit large triples, start index 10 .. 12)."""
    return random_groups(5, 2600 if long else 6, 10, 10, 12, p_run=0.3, p_step=0.02)


def _tail_index(groups, start):
    return start + sum(g[1] for g in groups)


def _valid():
    z = {}
    for h in WALK_HEADERS:
        z[f"index_walk_{h}"] = lambda h=h: _frame(h, FIRSTIDX, index_walk_groups(), 101)
    for tag, p in WALK_PRECISIONS.items():
        z[f"index_walk_w72_{tag}"] = lambda p=p: _frame("w72", FIRSTIDX, index_walk_groups(), 101, precision=p)
    for k, h in enumerate(EDGE_HEADERS):
        for s in (52, 53):
            z[f"bitsize_edges_{h}_i{s}"] = lambda k=k, h=h, s=s: _frame(
                h, s, random_groups(200 + k, 50, s, s, s, p_run=0.6, p_step=0.0), 300 + 2 * k + s)
    for c in CLEAN_C:
        z[f"clean_{c}_max"] = lambda c=c: _frame("a96", LASTIDX, _clean_c_groups(c, 10), 400 + c)
        z[f"clean_{c}_min"] = lambda c=c: _frame("w1", FIRSTIDX, _clean_c_groups(c, 0), 500 + c)
    z["all_flagged"] = lambda: _frame("a96", LASTIDX, [(10, 0)] * 130, 600, flag_all=True)
    for n in WORD_PER_ATOM:
        z[f"word_per_atom_{n}"] = lambda n=n: _frame("w31", 20, [(0, 0)] * n, 700 + n)
    z["drift33"] = lambda: _frame("w32", 20, [(0, 0)] * 4700, 800)
    z["mixed"] = lambda: _frame("w38", 24, random_groups(900, MIXED_N, 24, FIRSTIDX, LASTIDX), 901)
    z["idle_at_8"] = lambda: _frame("w38", 10, _idle_at_8_groups(), 1000)
    z["runs_0_to_10"] = lambda: _frame("w38", 30, RUNS_0_TO_10, 1100)
    for long in (False, True):  # the exact-length twins of nbytes-1_flagged_*
        z[f"exact_flagged_{'long' if long else 'short'}"] = lambda long=long: _frame(
            "w38", 10, _lead(long) + [(3, 0)] * 8 + [(3, 0, True)], 1200)
    return z


def _broken():
    """name -> builder; every name in a 40-atom ("short") and a "long" form
    whose defect is the last thing in a stream longer than 4,608 words."""
    z = {}
    for long in (False, True):
        s = "long" if long else "short"
        lead = _lead(long)
        clean_tail = lead + [(3, 0, True)] + [(3, 0)] * 8
        z[f"nbytes-1_clean_{s}"] = lambda g=clean_tail: _frame("w38", 10, g, 1201, nbytes_delta=-1)
        z[f"nbytes-8_clean_{s}"] = lambda g=clean_tail: _frame("w38", 10, g, 1201, nbytes_delta=-8)
        flagged_tail = lead + [(3, 0)] * 8 + [(3, 0, True)]  # the groups and seed of exact_flagged_*
        z[f"nbytes-1_flagged_{s}"] = lambda g=flagged_tail: _frame("w38", 10, g, 1200, nbytes_delta=-1)
        z[f"run_past_natoms_{s}"] = lambda g=clean_tail: _frame(
            "w38", 10, g, 1202, declared_natoms=sum(1 + x[0] for x in g) - 2)
        z[f"ends_before_natoms_{s}"] = lambda g=clean_tail: _frame(
            "w38", 10, g, 1203, declared_natoms=sum(1 + x[0] for x in g) + 50)
        flat = [(x[0], 0) for x in lead]  # no index steps: the helper walks down from 10 itself
        z[f"run_at_8_{s}"] = lambda g=flat: run_at_index_8(*HEADERS["w38"], 1000.0, Values(1204), g)
        down = lead + [(0, -1)] * (_tail_index(lead, 10) - 8) + [(0, 0)] * 30
        z[f"index_to_7_{s}"] = lambda g=down: _frame("w38", 10, g + [(0, -1)], 1205)
        up = flat[:450] + [(2, 1)] + [(2, 0)] * 12  # wide small triples: fewer groups pass word 4,608
        z[f"index_to_73_{s}"] = lambda g=up: _frame("w38", 71, g + [(2, 1)], 1206)
    return z


VALID = _valid()
BROKEN = _broken()
BROKEN_CLASSES = sorted({n.rsplit("_", 1)[0] for n in BROKEN})


@functools.lru_cache(maxsize=None)
def stream(name):
    """The named frame, built once per process."""
    return (VALID.get(name) or BROKEN[name])()


@functools.lru_cache(maxsize=None)
def expected(name):
    f = stream(name)
    return expected_angstrom(f.ints, f.precision)


def shared_natoms_frames(n_groups=1400, seed=1300):
    """One group list under three kinds of header (packed <= 52 bits, packed
    wider, per axis) and start indices: frames of one atom count with
    different streams, for a file or a launch of several records."""
    g = random_groups(seed, n_groups, 30, 26, 60)
    return [_frame("w38", 30, g, seed + 1), _frame("w72", 33, g, seed + 2), _frame("a32x", 28, g, seed + 3)]


def mixed_launch_frames():
    """(long valid, the same groups broken at the end, short valid): equal atom
    counts, different headers, lengths and validity.  The first two pass word
    4,608; the third (1-bit large triples, the indices 17 lower) is the
    shortest stream those groups have."""
    g = random_groups(1400, 1200, 30, 26, 60)
    return [_frame("w72", 30, g, 1401), _frame("a32x", 30, g, 1402, nbytes_delta=-1), _frame("w1", 13, g, 1403)]


# -- reach: what each stream is for, asserted from its layout ---------------------------

def _batch_pos(frame, k):
    return k % BATCH


def check_reach(name):
    f = stream(name)
    L = f.layout
    assert f.n_atoms == sum(1 + g.nsmall for g in L) and f.stream_bits == L[-1].bit + L[-1].nbits
    if name in VALID:
        assert f.nbytes == (f.stream_bits + 7) // 8 and f.declared == f.n_atoms and f.n_words <= 25000
    if name.startswith("index_walk"):
        assert run_widths(f) == set(range(FIRSTIDX, LASTIDX + 1)) and {52, 53} <= run_widths(f)
        for idx in range(FIRSTIDX, LASTIDX + 1):  # two clean groups with a run at every index
            assert sum(1 for g in L if g.idx == idx and g.nsmall > 0 and not g.flagged) >= 2, idx
        assert {g.nsmall for g in L} == set(range(1, 11))
        assert 1000 <= f.n_atoms <= 2000 and f.n_words > 2 * STAGE_WORDS
    elif name.startswith("bitsize_edges"):
        h, s = name[len("bitsize_edges_"):].rsplit("_i", 1)
        assert f.large_bits == LARGE_BITS[h] and len(L) == 50
        assert {g.idx for g in L} == {int(s)} and sum(g.nsmall for g in L) > 100 and max(g.nsmall for g in L) >= 9
    elif name.startswith("clean_"):
        c = int(name.split("_")[1])
        assert clean_stretches(f) == [c, c]
        mid = [k for k, g in enumerate(L) if g.flagged][-1]
        assert mid == c + 2 and _batch_pos(f, mid) != 0
        D = {g.nbits for g in L if not g.flagged}
        if name.endswith("_max"):
            assert D == {96 + 1 + 10 * 72} and BATCH * 817 > 32 * SCAN_WORDS  # the scan stops at the ring limit
        else:
            assert D == {2}
    elif name == "all_flagged":
        assert len(L) >= 130 and all(g.flagged and g.nbits == 822 for g in L)
        assert len(L) % BATCH != 0 and BATCH * 822 // 32 == 1644
    elif name.startswith("word_per_atom"):
        n = int(name.rsplit("_", 1)[1])
        assert f.n_words == n == f.n_atoms and all(g.nbits == 32 and not g.flagged for g in L)
    elif name == "drift33":
        assert all(g.nbits == 33 for g in L) and straddles(f, RING_WORDS) and f.n_words > LONG_WORDS
        assert {g.bit % 32 for g in L} == set(range(32))
    elif name == "mixed":
        assert 3000 <= len(L) <= 6000 and f.n_words > 2 * RING_WORDS
        assert straddles(f, RING_WORDS) and straddles(f, 2 * RING_WORDS)
        st = clean_stretches(f)
        assert sum(1 for n in st if n >= 2) > 100 and isolated_flags(f) > 100 and max(st) > 10
        assert {g.nsmall for g in L} == set(range(11)) and len(run_widths(f)) > 10
    elif name == "idle_at_8":
        at8 = [g for g in L if g.idx == 8]
        assert len(at8) > BATCH and all(g.nsmall == 0 for g in at8) and any(g.flagged for g in at8)
        last8 = max(k for k, g in enumerate(L) if g.idx == 8)
        assert L[last8 + 1].idx == 9 and L[last8 + 1].nsmall > 0  # back up, and a run opens
    elif name == "runs_0_to_10":
        assert [g.nsmall for g in L] == list(range(11)) and f.n_atoms == 66
    elif name.startswith("exact_flagged"):
        assert L[-1].flagged and not L[-2].flagged
    else:
        cls = name.rsplit("_", 1)[0]
        assert cls in BROKEN_CLASSES
        if cls.startswith("nbytes"):
            assert 8 * f.nbytes < f.stream_bits and 8 * f.nbytes > L[-3].bit  # cut inside the last groups
            assert L[-1].flagged == ("flagged" in cls) and not L[-2].flagged
            defect = 8 * f.nbytes
        elif cls == "run_past_natoms":
            assert L[-1].atom < f.declared < f.n_atoms and L[-1].nsmall >= 2
            defect = L[-1].bit
        elif cls == "ends_before_natoms":
            # the last byte's spare bits (< 8) cannot hold one of the 50 missing atoms (>= 39 bits each)
            assert f.declared == f.n_atoms + 50 and f.large_bits + 1 > 7 and 8 * f.nbytes - f.stream_bits < 8
            defect = f.stream_bits
        elif cls == "run_at_8":
            assert L[-1].idx == 8 and L[-1].nsmall == 2 and L[-2].nsmall == 0
            defect = L[-1].bit
        elif cls == "index_to_7":
            assert L[-1].idx == 8 and L[-1].flagged and all(g.idx >= 8 for g in L)
            defect = L[-1].bit
        else:
            assert cls == "index_to_73" and L[-1].idx == LASTIDX and L[-1].flagged
            defect = L[-1].bit
        if name.endswith("_long"):
            assert defect > 32 * LONG_WORDS and len(L) > 4 * BATCH  # batches written, the ring wrapped
        else:
            assert f.n_atoms <= 120 and f.n_words < STAGE_WORDS
