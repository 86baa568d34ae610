"""The two forms of csrc/metrics.hip restated for the tests -- a helper, not a test module.

``launch_metrics_t`` serves a call in one of two forms: 16-byte aligned u8 with at least one full
8192-sample block in ONE launch (metrics_prep + metrics_leaf_kernel), everything else in PARTS
(metrics_blocks / metrics_blocks_any<T> once per part, the chain of part k - 1 as workgroup 0 of
launch k, then metrics_ragged<T> and metrics_final).  This module states, once:

* ``sums_ref(yi, yf)``: the eight values out[0..7] of the device entry straight from NumPy (the
  reference's own reductions, before its ``/ n`` and ``sqrt`` hide a last-bit error);
* ``part_bounds(nbf)`` / ``launches_of(n, dtype, ideal_ptr, fixed_ptr)``: the parts and the launches
  of one call, in order, as (kernel, template arguments, grid.x);
* a PERIODIC reference: a pattern of P = 509 full blocks tiled to n samples.  NumPy sums a
  contiguous float64 array in 8192-element blocks added in order to 0.0, so the sum of the tiled
  array is the in-order chain over the pattern's per-block ``np.add.reduce`` values, tiled, with
  the ragged slice's ``np.add.reduce`` added last; counts multiply out, the max is the pattern's.
  509 is prime and shares no factor with 4, 512, 2048 or 8192 (waves per workgroup, block sums per
  chain group, the part sizes): a block read at a wrong stride, group or part offset is a block of
  another residue, and the pattern's 509 block sums are pairwise distinct;
* ``mutants``: the orders a wrong parts form would add in (the running sum reset at a part boundary,
  parts chained in reverse, two chain groups swapped, a block dropped or repeated at a part
  boundary, the ragged sum first), for the CPU test that proves the reference tells them apart;
* ``ROWS`` / ``FORMS``: the pinned sizes, each the smallest n that reaches what it names;
* the hypothesis strategy of tests/test_gpu_metrics_forms.py, route first, built by construction.

The fill is d = fixed - ideal signed with magnitudes spread over 2^-30 .. 2^30 and a pattern sum
of zero (see ``pattern``): the signed sum's running value keeps changing exponent, so a change of
order changes bits (all-positive sums absorb an early difference as the running sum's ulp grows;
tests/test_metrics_cases.py records which mutants sum|d| and sum d^2 see).  A given reordering
still leaves sum d unchanged for about one seed in thirty, so SEED is the first seed (from 1 up:
15; 17 and 19 do too) for which all 141 mutants of the seven pinned sizes change sum d -- chosen
on the CPU from the reference alone.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

# the constants of metrics.hip / fir_common.h (tests/test_metrics_cases.py reads them back)
CONSTANTS = {"kTailPart": 2048, "kBodyPart": 8192, "kMaxParts": 16, "kMetricBlocks": 512, "kMetricPBlocks": 256,
             "kMetricPrepBlocks": 64, "kPwBlock": 8192, "kChainDepth": 8, "kWave": 64, "kBlock": 256}
PW = CONSTANTS["kPwBlock"]
TAIL, BODY, MAX_PARTS = CONSTANTS["kTailPart"], CONSTANTS["kBodyPart"], CONSTANTS["kMaxParts"]
WAVES = CONSTANTS["kBlock"] // CONSTANTS["kWave"]           # waves (= blocks in flight) per workgroup
GROUP = CONSTANTS["kChainDepth"] * CONSTANTS["kWave"]       # block sums per chain group
CNT_SLOTS = MAX_PARTS * CONSTANTS["kMetricBlocks"] + 1

# template argument of metrics_blocks_any / metrics_ragged / metrics_prep as the demangler writes it
TARG = {"uint8": "unsigned char", "int8": "signed char", "uint16": "unsigned short", "int16": "short",
        "uint32": "unsigned int", "int32": "int", "uint64": "unsigned long", "int64": "long",
        "float16": "_Float16", "float32": "float", "float64": "double"}
DTYPES = tuple(TARG)          # uint8 first
OTHER_DTYPES = DTYPES[1:]     # the ten that never take the u8 kernels


def _dt(dtype) -> str:
    name = np.dtype(dtype).name
    return "uint8" if name == "bool" else name  # bool goes as its bytes


# ---- the reference ---------------------------------------------------------------------------------
def sums_ref(yi, yf) -> np.ndarray:
    """out[0..7] of fir_compare_metrics_dev from NumPy: max|d| (NaN propagates), np.add.reduce of
    |d|, d^2 and d over the flat float64 arrays, #(fixed == 0), #(fixed == 255),
    #(ideal < 0 or ideal > 255), n."""
    ideal = np.ascontiguousarray(yi, dtype=np.float64).reshape(-1)
    fx = np.ascontiguousarray(yf).reshape(-1)
    d = fx.astype(np.float64) - ideal
    ad = np.abs(d)
    n = ideal.size
    return np.array([np.max(ad) if n else 0.0, np.add.reduce(ad), np.add.reduce(np.square(d)), np.add.reduce(d),
                     np.count_nonzero(fx == 0), np.count_nonzero(fx == 255),
                     np.count_nonzero((ideal < 0.0) | (ideal > 255.0)), n], dtype=np.float64)


def differing(got, want) -> list:
    """Indices where two float64 vectors differ bit for bit (the sign of zero counts; NaN = NaN)."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert g.shape == w.shape
    same = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
    return [int(i) for i in np.flatnonzero(~same)]


def describe(got, want) -> str:
    return "; ".join(f"out[{i}] = {float(got[i])!r} ({float(got[i]).hex()}), want {float(want[i])!r} "
                     f"({float(want[i]).hex()})" for i in differing(got, want))


# ---- launch_metrics_t ------------------------------------------------------------------------------
def part_bounds(nbf: int) -> list:
    """bounds[0..nparts] of the full blocks: sizes taken from the END (kTailPart last, kBodyPart
    before it, the first part the rest, at most kMaxParts)."""
    sizes, left = [], nbf
    while left > 0:
        want = TAIL if not sizes else BODY
        take = left if len(sizes) == MAX_PARTS - 1 or left <= want else want
        sizes.append(take)
        left -= take
    bounds = [0]
    for s in reversed(sizes):
        bounds.append(bounds[-1] + s)
    return bounds


def one_launch(n: int, dtype, ideal_ptr: int, fixed_ptr: int) -> bool:
    return _dt(dtype) == "uint8" and ideal_ptr % 16 == 0 and fixed_ptr % 16 == 0 and n // PW > 0


def launches_of(n: int, dtype, ideal_ptr: int, fixed_ptr: int) -> list:
    """The launches of one call in order: (kernel, template arguments, grid.x)."""
    name = _dt(dtype)
    t, nbf = (TARG[name],), n // PW
    if one_launch(n, dtype, ideal_ptr, fixed_ptr):
        g = min(CONSTANTS["kMetricPBlocks"], -(-nbf // WAVES))
        return [("metrics_prep", t, CONSTANTS["kMetricPrepBlocks"]), ("metrics_leaf_kernel", (), g + 1)]
    out, b = [], part_bounds(nbf)
    for k in range(len(b) - 1):
        g = min(CONSTANTS["kMetricBlocks"], -(-(b[k + 1] - b[k]) // WAVES))
        grid = g + (1 if k else 0)  # + the workgroup that chains part k - 1
        out.append(("metrics_blocks", (), grid) if name == "uint8" else ("metrics_blocks_any", t, grid))
    if n % PW:
        out.append(("metrics_ragged", t, 1))
    return out + [("metrics_final", (), 1)]


def cnt_slots_used(n: int) -> int:
    """Cnt slots the parts form writes (one per streaming workgroup, one for the ragged block)."""
    b = part_bounds(n // PW)
    return sum(min(CONSTANTS["kMetricBlocks"], -(-(b[k + 1] - b[k]) // WAVES)) for k in range(len(b) - 1)) + (1 if n % PW else 0)


# ---- the periodic pattern --------------------------------------------------------------------------
P = 509
SEED = 15


def spread_fill(rng, n: int):
    """(ideal, fixed u8): d = fixed - ideal signed, |d| spread over 2^-30 .. 2^30."""
    yf = rng.integers(0, 256, n, dtype=np.uint8)
    yi = yf - rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))
    return yi, yf


@functools.lru_cache(maxsize=2)
def pattern(seed: int = SEED):
    """(ideal float64, fixed uint8) of P full blocks: the spread fill, its last sample's d set to
    minus the sum of all others.  Tiled, a pattern whose sum d is T adds T every period: the running
    sum grows linearly (2^46 after 245 periods), its ulp with it, and a rounding difference made
    early -- two groups swapped in the first part -- is absorbed before the end (seen here: 16 of 16
    such swaps of the 16-part row left sum d unchanged).  With T = 0 to within roundings the running
    sum d walks through the binades up to 2^38 and back to nearly 0 in every period, so the grid an
    add rounds on depends on what was added before it, and the sum never outgrows a difference once
    made.  (Held in ONE binade by a large first sample the sum is fixed-point arithmetic, which no
    reordering changes: that was tried too.)"""
    yi, yf = spread_fill(np.random.default_rng(seed), P * PW)
    d = yf.astype(np.float64) - yi
    yi[-1] = yf[-1] + float(np.sum(d[:-1]))  # the last d = -T to within roundings
    yi.setflags(write=False)
    yf.setflags(write=False)
    return yi, yf


@dataclass(frozen=True)
class Blocks:
    sums: np.ndarray   # [3][P]: np.add.reduce of |d|, d^2, d over each block
    mx: np.ndarray     # [P] max|d|
    cnt: np.ndarray    # [3][P]: #(fixed == 0), #(fixed == 255), #(ideal out of [0, 255])


def _terms(yi, yf):
    d = yf.astype(np.float64) - yi
    return np.abs(d), np.square(d), d


@functools.lru_cache(maxsize=2)
def pattern_blocks(seed: int = SEED) -> Blocks:
    yi, yf = pattern(seed)
    arrs = [a.reshape(P, PW) for a in _terms(yi, yf)]
    sums = np.array([[np.add.reduce(a[b]) for b in range(P)] for a in arrs])  # one 1-D reduce per block
    f, i = yf.reshape(P, PW), yi.reshape(P, PW)
    cnt = np.array([(f == 0).sum(1), (f == 255).sum(1), ((i < 0.0) | (i > 255.0)).sum(1)], dtype=np.int64)
    return Blocks(sums, arrs[0].max(1), cnt)


def chain(seq, start: float = 0.0) -> float:
    """start + seq[0] + seq[1] + ... in order, each add rounded."""
    return float(np.add.accumulate(np.concatenate(([start], np.asarray(seq, np.float64))))[-1])


def ragged_slice(n: int, seed: int = SEED):
    """(ideal, fixed) of the tiled array's ragged last block [nbf * 8192, n)."""
    yi, yf = pattern(seed)
    nbf, m = divmod(n, PW)
    o = nbf % P * PW
    return yi[o:o + m], yf[o:o + m]


def block_seq(n: int, seed: int = SEED):
    """([3][nbf] block sums of the tiled array in order, [3] ragged sums or None)."""
    nbf, m = divmod(n, PW)
    seq = pattern_blocks(seed).sums[:, np.arange(nbf) % P]
    r = np.array([np.add.reduce(a) for a in _terms(*ragged_slice(n, seed))]) if m else None
    return seq, r


def periodic_ref(n: int, seed: int = SEED) -> np.ndarray:
    """sums_ref of the pattern tiled to n samples, without the array."""
    nbf, m = divmod(n, PW)
    pb = pattern_blocks(seed)
    seq, r = block_seq(n, seed)
    sums = [chain(seq[a]) for a in range(3)]
    reps, rem = divmod(nbf, P)
    cnt = reps * pb.cnt.sum(1) + pb.cnt[:, :rem].sum(1)
    mx = pb.mx[:min(nbf, P)].max() if nbf else 0.0
    if m:
        ri, rf = ragged_slice(n, seed)
        sums = [s + float(v) for s, v in zip(sums, r)]  # the ragged block's sum is the last in order
        cnt = cnt + np.array([(rf == 0).sum(), (rf == 255).sum(), ((ri < 0.0) | (ri > 255.0)).sum()])
        mx = max(mx, np.abs(rf.astype(np.float64) - ri).max())
    return np.array([mx, *sums, *cnt, n], dtype=np.float64)


def tiled(n: int, seed: int = SEED):
    """The pattern tiled to n samples, materialised on the host."""
    yi, yf = pattern(seed)
    return np.resize(yi, n), np.resize(yf, n)


# ---- mutant orders ---------------------------------------------------------------------------------
def mutants(seq, r, bounds):
    """(name, value) of the sums a wrong parts form would give for ONE array: ``seq`` its block sums
    in order, ``r`` its ragged sum (None: no ragged block), ``bounds`` the part bounds.  Boundary
    mutants at every inner bound; one group swap per part with two full groups (its first two)."""
    seq = np.asarray(seq, np.float64)
    fin = (lambda s: s) if r is None else (lambda s: s + float(r))
    inner = bounds[1:-1]
    for b in inner:
        yield f"reset@{b}", fin(chain(seq[b:]))  # the running sum back to 0.0 where a part starts
    if inner:
        order = [seq[bounds[k]:bounds[k + 1]] for k in reversed(range(len(bounds) - 1))]
        yield "parts_reversed", fin(chain(np.concatenate(order)))
    for k in range(len(bounds) - 1):
        lo = bounds[k]
        if bounds[k + 1] - lo >= 2 * GROUP:
            s = seq.copy()
            s[lo:lo + GROUP], s[lo + GROUP:lo + 2 * GROUP] = seq[lo + GROUP:lo + 2 * GROUP], seq[lo:lo + GROUP]
            yield f"groups_swapped@{lo}", fin(chain(s))
    for b in inner:
        for at in (b - 1, b):  # the last block of the earlier part, the first of the later
            yield f"dropped@{at}", fin(chain(np.delete(seq, at)))
            yield f"repeated@{at}", fin(chain(np.insert(seq, at, seq[at])))
    if r is not None:
        yield "ragged_first", chain(seq, 0.0 + float(r))


# ---- the pinned sizes ------------------------------------------------------------------------------
@dataclass(frozen=True)
class Row:
    nbf: int
    m: int
    ref: str        # "numpy" (materialised), "periodic" or "both"
    reaches: str

    @property
    def n(self) -> int:
        return self.nbf * PW + self.m

    @property
    def id(self) -> str:
        return f"nbf{self.nbf}+{self.m}"


ROWS = (
    Row(TAIL, 0, "numpy", "one part of exactly kTailPart; g = 512, one block per wave; no ragged launch; "
                          "metrics_final chains 4 full groups"),
    Row(TAIL + 1, 1, "numpy", "two parts; the in-launch chain of a 1-block part; the carry into metrics_final"),
    Row(TAIL + GROUP + 1, 129, "numpy", "in-launch chain of one full group + 1 (add_group's full path, then its tail)"),
    Row(TAIL + 4 * CONSTANTS["kMetricBlocks"] + 1, 4321, "both",
        "first part past 512 * 4 blocks: g capped; wave 0's second grid-stride iteration"),
    Row(TAIL + BODY, 0, "periodic", "a body part of exactly kBodyPart: 4 blocks per wave, 16 full groups in-launch"),
    Row(TAIL + BODY + 1, 7, "periodic", "three parts: state[] read by an in-launch chain (lo != 0)"),
    Row(TAIL + (MAX_PARTS - 2) * BODY + BODY + 1, 4321, "periodic",
        "16 parts; the nparts == kMaxParts - 1 clause with a rest larger than kBodyPart; Cnt slot 8192 (the last) "
        "written by metrics_ragged"),
)
SMALL_ROWS_MAX = TAIL + 4 * CONSTANTS["kMetricBlocks"] + 1  # rows up to here also run the two extra forms


@dataclass(frozen=True)
class Form:
    name: str
    dtype: str
    ideal_lead: int
    fixed_lead: int
    every_row: bool


FORMS = (
    Form("u8_fixed_off1", "uint8", 0, 1, True),    # metrics_blocks
    Form("i16", "int16", 0, 0, True),              # metrics_blocks_any<short>
    Form("f64", "float64", 0, 0, False),           # metrics_blocks_any<double>: the widest loads
    Form("u8_ideal_off8", "uint8", 8, 0, False),   # metrics_blocks by the other half of `vec`
)
TWIN = Form("twin_u8_aligned", "uint8", 0, 0, True)  # the same data through the one-launch form


def pinned_cases():
    return [(row, form) for row in ROWS for form in FORMS if form.every_row or row.nbf <= SMALL_ROWS_MAX]


@functools.lru_cache(maxsize=None)
def row_refs(row: Row) -> tuple:
    """The references a row is held against: ((how, out[0..7]), ...)."""
    refs = []
    if row.ref in ("numpy", "both"):
        refs.append(("numpy", sums_ref(*tiled(row.n))))
    if row.ref in ("periodic", "both"):
        refs.append(("periodic", periodic_ref(row.n)))
    for _, v in refs:
        v.setflags(write=False)
    return tuple(refs)


# ---- the byte pairs of the one-launch form's counts --------------------------------------------------
def byte_pairs(shift: int):
    """(ideal, fixed u8) of 16 blocks whose fixed bytes hold all 65,536 ordered byte pairs (a, b at
    2 (256 a + b)), rotated by `shift` bytes: at shift 1 every pair also straddles a dword edge."""
    a = np.arange(256, dtype=np.uint8)
    yf = np.roll(np.stack([np.repeat(a, 256), np.tile(a, 256)], axis=1).reshape(-1), shift)
    rng = np.random.default_rng(65536 + shift)
    yi = yf - rng.standard_normal(yf.size) * np.exp2(rng.integers(-30, 31, yf.size))
    return yi, yf


# ---- the property test's cases -----------------------------------------------------------------------
ROUTES = ("leaf", "parts:u8", "parts:any", "ragged_only", "empty")
U8_OFF = ("ideal8", "fixed1", "both")
FILLS = ("spread", "image", "sat:0", "sat:255", "sat:min", "sat:max", "exact:0", "exact:-0")
NBF_EDGES = (1, 3, 4, 5, 8, 9)
M_EDGES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 255, 256, 257, 1023, 1024, 1025, 4095, 4096,
           4097, 8191)
ALL_DTYPES = DTYPES + ("bool",)
MAX_EXAMPLES = 400  # of the property test
ROUTE_DRAW = ("leaf",) * 2 + ("parts:u8",) * 3 + ("parts:any",) * 4 + ("ragged_only",) * 4 + ("empty",)  # the route's odds


def variants():
    """Every (route, variant) the property test must have run."""
    out = [("leaf", "uint8")] + [("parts:u8", v) for v in U8_OFF]
    out += [("parts:any", d) for d in OTHER_DTYPES] + [("parts:any", "bool")]
    out += [("ragged_only", d) for d in ALL_DTYPES] + [("empty", d) for d in ("uint8", "int16", "float64")]
    return out


@dataclass(frozen=True)
class Case:
    route: str
    variant: str
    dtype: str
    nbf: int
    m: int
    ideal_lead: int
    fixed_lead: int
    fill: str
    seed: int

    @property
    def n(self) -> int:
        return self.nbf * PW + self.m


def forms_case():
    """hypothesis strategy: the route first, then a call built to take it (no assume, no filter)."""
    from hypothesis import strategies as st

    @st.composite
    def build(draw):
        route = draw(st.sampled_from(ROUTE_DRAW))
        variant = draw(st.sampled_from([v for r, v in variants() if r == route]))
        dtype = "uint8" if route in ("leaf", "parts:u8") else variant
        size = np.dtype(dtype).itemsize
        full = st.one_of(st.sampled_from(NBF_EDGES), st.integers(1, 40))
        m_any = st.one_of(st.sampled_from(M_EDGES), st.integers(0, PW - 1))
        lead16 = st.sampled_from((0, 16, 48, 256))
        if route == "empty":
            nbf, m = 0, 0
        elif route == "ragged_only":
            nbf, m = 0, draw(st.one_of(st.sampled_from(M_EDGES[1:]), st.integers(1, PW - 1)))
        else:
            nbf, m = draw(full), draw(m_any)
        if route == "leaf":
            il, fl = draw(lead16), draw(lead16)
        elif route == "parts:u8":
            il = draw(lead16) + (8 if variant in ("ideal8", "both") else 0)
            fl = draw(lead16) + (draw(st.integers(1, 15)) if variant in ("fixed1", "both") else 0)
        elif variant == "bool":  # bool goes as u8: off 16 it takes the parts (launches_of says which kernels)
            il, fl = draw(lead16), draw(lead16) + (draw(st.integers(1, 15)) if route == "parts:any" else draw(st.integers(0, 15)))
        else:
            il, fl = draw(st.sampled_from((0, 8, 16, 24))), draw(st.integers(0, 31)) * size % 256
        return Case(route, variant, dtype, nbf, m, il, fl, draw(st.sampled_from(FILLS)), draw(st.integers(0, 2**20)))

    return build()


def route_kernels(c: Case) -> list:
    """The kernels the route of a drawn case stands for, in launch order."""
    blocks = "metrics_blocks" if c.dtype in ("uint8", "bool") else "metrics_blocks_any"
    tail = ["metrics_ragged"] * (c.m > 0) + ["metrics_final"]
    return {"leaf": ["metrics_prep", "metrics_leaf_kernel"], "empty": ["metrics_final"], "ragged_only": tail,
            "parts:u8": ["metrics_blocks"] + tail, "parts:any": [blocks] + tail}[c.route]


def pinned_examples() -> list:
    """One case per (route, variant), run ahead of the drawn ones: whatever is drawn, every route and
    every dtype runs once.  Sizes, fills and leads cycle through the edges."""
    out = []
    for i, (route, variant) in enumerate(variants()):
        dtype = "uint8" if route in ("leaf", "parts:u8") else variant
        size = np.dtype(dtype).itemsize
        nbf = 0 if route in ("ragged_only", "empty") else NBF_EDGES[i % len(NBF_EDGES)]
        m = 0 if route == "empty" else M_EDGES[1 + 5 * i % (len(M_EDGES) - 1)]
        il = 8 if variant in ("ideal8", "both") else 0
        fl = 0 if route == "leaf" or variant == "ideal8" else (1 + 2 * i % 15 if size == 1 else size * (i % 3))
        out.append(Case(route, variant, dtype, nbf, m, il, fl, FILLS[i % len(FILLS)], i))
    return out


def _span(dtype: str):
    """The dtype's values the fills draw from: within [-300, 300], so 0 and 255 occur where it has them."""
    if dtype == "bool":
        return 0, 1
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return -300, 300
    info = np.iinfo(dt)
    return max(int(info.min), -300), min(int(info.max), 300)


def _extreme(dtype: str, top: bool):
    if dtype == "bool":
        return top
    dt = np.dtype(dtype)
    if dt.kind == "f":  # float64: 2^500, whose square still sums without overflow (no non-finite value here)
        v = 2.0 ** 500 if dt.itemsize == 8 else float(np.finfo(dt).max)
        return v if top else -v
    return int(np.iinfo(dt).max if top else np.iinfo(dt).min)


def make_data(c: Case):
    """(ideal float64, fixed of c.dtype) of a drawn case."""
    rng = np.random.default_rng(c.seed)
    n, dt = c.n, np.dtype(c.dtype)
    lo, hi = _span(c.dtype)

    def values():  # a mix that holds 0 and 255 (where the dtype has them) often enough to count
        v = rng.integers(lo, hi + 1, n)
        pick = rng.integers(0, 8, n)
        v = np.where(pick == 0, 0, np.where(pick == 1, min(hi, 255), v))
        if dt.kind == "f":
            return (v + rng.integers(0, 2, n) * 0.5).astype(dt)
        return v.astype(dt)

    if c.fill == "spread":
        yf = values()
        yi = yf.astype(np.float64) - rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))
    elif c.fill == "image":
        yi = rng.uniform(-64.0, 320.0, n)
        near = np.rint(yi) + rng.integers(-3, 4, n)
        yf = (near > 128) if c.dtype == "bool" else np.clip(near, max(lo, 0), min(hi, 255)).astype(dt)
    elif c.fill.startswith("sat:"):
        yi = rng.uniform(-64.0, 320.0, n)
        what = c.fill[4:]
        v = {"0": 0, "255": min(hi, 255), "min": _extreme(c.dtype, False), "max": _extreme(c.dtype, True)}[what]
        yf = np.full(n, v, dtype=dt)
    elif c.fill == "exact:0":  # d == 0 everywhere
        yf = values()
        yi = yf.astype(np.float64)
    else:  # "exact:-0": a float fixed of -0.0 against +0.0 gives d = -0.0; an integer 0 against -0.0 gives +0.0
        yf = np.full(n, -0.0 if dt.kind == "f" else 0, dtype=dt)
        yi = np.full(n, 0.0 if dt.kind == "f" else -0.0)
    return np.ascontiguousarray(yi, dtype=np.float64), np.ascontiguousarray(yf)
