"""Seeded input families for the sampler tests (tests/test_oracle_sampling_rows.py on the CPU,
tests/test_gpu_sampling_rows.py on the GPU).  Every family returns Case objects: probs fp32 [bs, vocab] and the
per-row top_k / top_p / min_p arrays (None = that filter is switched off, a NULL pointer in the C ABI) and uniforms.
Nothing here touches a GPU; expected results come from oracle/sampling.py alone."""
import hashlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from oracle import sampling as osamp

WAVES = 16            # kSampWaves of csrc/sampling.hip: one id segment per wave
K_ALL = 1 << 30       # sampler.TOP_K_ALL
VOCAB_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 16 * 64 * 3 - 1, 16 * 64 * 3, 16 * 64 * 3 + 1,
               32000, 50257, 128256, 152064)
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))


def seg_len(vocab: int) -> int:
    """seg_len() of csrc/sampling.hip: ids per wave segment, a multiple of 64."""
    return (((vocab + WAVES - 1) // WAVES) + 63) & ~63


@dataclass
class Case:
    name: str
    probs: np.ndarray
    top_ks: Optional[np.ndarray]
    top_ps: Optional[np.ndarray]
    min_ps: Optional[np.ndarray]
    uniform: np.ndarray

    def __post_init__(self):
        bs = self.probs.shape[0]
        self.probs = np.ascontiguousarray(self.probs, dtype=np.float32)
        self.top_ks = None if self.top_ks is None else np.asarray(self.top_ks, dtype=np.int32).reshape(bs)
        self.top_ps = None if self.top_ps is None else np.asarray(self.top_ps, dtype=np.float32).reshape(bs)
        self.min_ps = None if self.min_ps is None else np.asarray(self.min_ps, dtype=np.float32).reshape(bs)
        self.uniform = np.asarray(self.uniform, dtype=np.float32).reshape(bs)

    @property
    def bs(self):
        return self.probs.shape[0]

    @property
    def vocab(self):
        return self.probs.shape[1]

    def params(self, b):
        """(top_k, top_p, min_p) of row b, None where the filter is off."""
        return (None if self.top_ks is None else int(self.top_ks[b]),
                None if self.top_ps is None else float(self.top_ps[b]),
                None if self.min_ps is None else float(self.min_ps[b]))

    def loop_params(self, b):
        """The same for the loop form of the oracle, which has no 'off': a top_k above any vocabulary,
        a top_p above any row's mass (fx sums stay below 2^49 = fx(2.0)), a zero floor."""
        k, p, m = self.params(b)
        return (1 << 40 if k is None else k, 4.0 if p is None else p, 0.0 if m is None else m)


def _seed(*key) -> int:
    return int.from_bytes(hashlib.blake2b(repr(key).encode(), digest_size=4).digest(), "little")


# --------------------------------------------------------------------------- expected results
def expected(case: Case):
    """(keep bool[bs, vocab], totals uint64[bs], ids int64[bs], renorm fp32[bs, vocab]) from the vectorised oracle.
    Equal (row, parameters) pairs inside a case are computed once - every row is still compared."""
    keep = np.zeros(case.probs.shape, dtype=bool)
    totals = np.zeros(case.bs, dtype=np.uint64)
    local = {}
    for b in range(case.bs):
        key = (hashlib.blake2b(case.probs[b].tobytes(), digest_size=16).digest(), case.params(b))
        if key not in local:
            one = lambda a: None if a is None else a[b:b + 1]
            k, t = osamp.select_rows(case.probs[b:b + 1], one(case.top_ks), one(case.top_ps), one(case.min_ps))
            local[key] = (k[0], t[0])
        keep[b], totals[b] = local[key]
    ids = osamp.sample_rows(case.probs, case.top_ks, case.top_ps, case.min_ps, case.uniform, selected=(keep, totals))
    ren = osamp.renorm_rows(case.probs, case.top_ks, case.top_ps, case.min_ps, selected=(keep, totals))
    return keep, totals, ids, ren


def cut_levels(case: Case):
    return [osamp.cut_level(case.probs[b], *case.params(b)) for b in range(case.bs)]


# --------------------------------------------------------------------------- a. model-shaped
SCALES = (0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 12.0)
TEMPS = (0.3, 0.7, 1.0, 1.5, 2.0)


def model_rows(vocab: int, rows: int, seed) -> np.ndarray:
    """softmax((randn * s).to(bf16 | fp16).float() / T) on the CPU: what the sampler sees behind a 16-bit LM head.
    Every third row is fp16-valued where that still leaves the row tie-heavy (distinct values < vocab / 8): a 10-bit
    mantissa gives ~11 000 - 16 000 distinct values, below the bound only from vocab 128256 up; bf16 gives ~2 800."""
    g = torch.Generator().manual_seed(_seed("model", vocab, seed))
    out = np.empty((rows, vocab), dtype=np.float32)
    for i in range(rows):
        s, t = SCALES[i % len(SCALES)], TEMPS[(i // 2) % len(TEMPS)]
        dt = torch.float16 if i % 3 == 0 and vocab >= 128256 else torch.bfloat16
        logits = (torch.randn(vocab, generator=g) * s).to(dt).float()
        out[i] = torch.softmax(logits / np.float32(t), dim=-1).numpy()
    return out


def model_params(vocab: int, rows: int, seed):
    """top-k only, top-p only, min-p only, all three - in turn."""
    r = np.random.default_rng(_seed("model_params", vocab, seed))
    ks = np.full(rows, K_ALL, dtype=np.int32)
    ps = np.ones(rows, dtype=np.float32)
    ms = np.zeros(rows, dtype=np.float32)
    k_choices = [1, 2, 7, 50, 64, 1000, 40000]
    p_choices = [0.2, 0.5, 0.9, 0.95, 0.99, 0.999]
    m_choices = [0.001, 0.01, 0.05, 0.3]
    for i in range(rows):
        mode = i % 4
        if mode in (0, 3):
            ks[i] = k_choices[r.integers(len(k_choices))]
        if mode in (1, 3):
            ps[i] = p_choices[r.integers(len(p_choices))]
        if mode in (2, 3):
            ms[i] = m_choices[r.integers(len(m_choices))]
    return ks, ps, ms, r.random(rows, dtype=np.float32)


def family_a(vocab: int, rows: int = 56, seed=0) -> Case:
    ks, ps, ms, u = model_params(vocab, rows, seed)
    return Case(f"a_model_v{vocab}", model_rows(vocab, rows, seed), ks, ps, ms, u)


def distinct_values(case: Case):
    return [int(np.unique(case.probs[b]).size) for b in range(case.bs)]


# --------------------------------------------------------------------------- b. tie plateaus
def plateau_row(vocab: int, tiny: bool, seed):
    """One plateau value on an id set that straddles the wave-segment edges, the 64-lane chunk edges, id 0 and the
    last id; up to three larger values above it; smaller values elsewhere.  All values above and on the plateau
    are powers of two, so every partial mass is a short binary fraction that a fp32 top_p can state exactly.
    tiny: the row scaled by 2^-24 (exact), which brings one unit of fx within reach of a fp32 top_p."""
    r = np.random.default_rng(_seed("plateau", vocab, tiny, seed))
    seg = seg_len(vocab)
    ids = {0, vocab - 1}
    for w in range(1, WAVES):
        ids.update(i for i in (w * seg - 2, w * seg - 1, w * seg, w * seg + 1))
    for c in (1, 2, 5):
        ids.update((64 * c - 1, 64 * c, 64 * c + 1, seg + 64 * c - 1, seg + 64 * c))
    ids = {i for i in ids if 0 <= i < vocab}
    low = min(vocab, 1 << 14)                                       # tops and filler ties sit at low ids
    cand = np.array([i for i in range(low) if i not in (0, vocab - 1)] or ([1] if vocab == 2 else []), dtype=np.int64)
    r.shuffle(cand)
    tops = np.sort(cand[:min(3, vocab // 4 + (vocab > 1))])
    ids -= set(int(t) for t in tops)
    want = min(200, vocab - len(tops))
    if len(ids) < want:
        ids.update(int(i) for i in [c for c in cand[len(tops):] if int(c) not in ids][:want - len(ids)])
    ids = np.array(sorted(ids), dtype=np.int64)
    n_top = len(tops)
    m = len(ids)
    q = np.float32(2.0 ** -max(int(np.ceil(np.log2(max(2 * m, 2)))), 5))   # m * q <= 1/2, q below the tops
    row = np.zeros(vocab, dtype=np.float32)
    rest = np.ones(vocab, dtype=bool)
    rest[ids] = False
    rest[tops] = False
    row[rest] = (r.random(int(rest.sum()), dtype=np.float32) * q * np.float32(0.5) / max(vocab, 1)).astype(np.float32)
    row[ids] = q
    row[tops] = [np.float32(2.0 ** -(2 + j)) for j in range(n_top)]
    if tiny:
        row = row * np.float32(2.0 ** -24)
    return row, ids, tops


def _u_at(row, keep, total, tok, edge):
    """A uniform whose draw r = floor(u * total) lands on token tok: in the first ("first") or last ("last") few
    units of its interval of the kept mass taken in id order - where one tie too many or too few on either side of it
    moves the draw to another token."""
    w = np.where(keep, osamp.fx(osamp.clean(row)), np.uint64(0))
    lo = int(w[:tok].sum(dtype=np.uint64))
    hi = lo + int(w[tok]) - 1
    r_of = lambda u: min(int(np.floor(np.float64(u) * np.float64(total))), total - 1)
    if edge == "first":
        u = np.float32(lo / total)
        while r_of(u) < lo:
            u = np.nextafter(u, np.float32(2))
    else:
        u = np.float32(min((hi + 1) / total, 1.0))
        while r_of(u) > hi:
            u = np.nextafter(u, np.float32(0))
    assert lo <= r_of(u) <= hi
    return u


def family_b(vocab: int, tiny: bool = False, seed=0):
    """-> (Case, intended ties kept per row).  Cuts by top_k and by top_p at 0, 1, 63, 64, 65 ties kept, around the
    tie count of the first segments, and all; by top_p with the boundary 'exclusive mass == fx(top_p)' hit exactly
    and missed by one step (tiny: by exactly one unit of fx); per cut, draws on the first kept tie, the last kept
    tie, the last token above the plateau and the kept token after the first dropped tie."""
    row, ids, tops = plateau_row(vocab, tiny, seed)
    m, n_top = len(ids), len(tops)
    seg = seg_len(vocab)
    w = int(osamp.fx(row[ids[:1]])[0])
    mass_above = int(osamp.fx(row[tops]).sum(dtype=np.uint64))
    in_seg0, in_seg01 = int((ids < seg).sum()), int((ids < 2 * seg).sum())
    counts = sorted({t for t in (0, 1, 63, 64, 65, in_seg0 - 1, in_seg0, in_seg0 + 1, in_seg01 - 1, in_seg01,
                                 in_seg01 + 1, m - 1, m) if 0 <= t <= m})
    cuts = []                                          # (top_k, top_p, intended ties kept)
    for t in counts:
        cuts.append((n_top + t, 1.0, t))
        # exclusive mass of the t-th tie (1-based) is mass_above + (t - 1) w: top_p exactly there keeps t ties
        e = mass_above + (t - 1) * w if t else mass_above - 1
        if e < 0:
            continue
        top_p = np.float32(e / osamp.FX_ONE)
        if int(np.floor(np.float64(top_p) * osamp.FX_ONE)) != e:
            continue                                   # (t = 0 on a row that is not tiny: one unit is out of reach)
        cuts.append((K_ALL, top_p, t))
        if t >= 1 and e > 0:                           # one step short of the boundary: the t-th tie goes
            below = np.float32((e - 1) / osamp.FX_ONE) if tiny else np.nextafter(top_p, np.float32(0))
            if tiny:
                assert int(np.floor(np.float64(below) * osamp.FX_ONE)) == e - 1
            cuts.append((K_ALL, below, t - 1))
    probs, ks, ps, us, intended = [], [], [], [], []
    for k, p, t in cuts:
        keep, total, _, _ = osamp._select_row(row, k, p, None)
        kept_ties, dropped_ties = ids[keep[ids]], ids[~keep[ids]]
        targets = []                                   # (token, edge of its interval)
        if len(kept_ties):
            targets += [(int(kept_ties[0]), "first"), (int(kept_ties[-1]), "last")]
        if n_top:
            targets.append((int(tops.max()), "last"))
        after = np.flatnonzero(keep[int(dropped_ties[0]) + 1:]) if len(dropped_ties) else []
        if len(after):                                 # the kept token that follows the first dropped tie
            targets.append((int(dropped_ties[0]) + 1 + int(after[0]), "first"))
        for tok, edge in targets or [(0, "first")]:
            probs.append(row)
            ks.append(k)
            ps.append(p)
            us.append(_u_at(row, keep, total, tok, edge) if total and keep[tok] and osamp.fx(row[tok:tok + 1])[0] else 0.5)
            intended.append(t)
    name = f"b_plateau{'_tiny' if tiny else ''}_v{vocab}"
    return Case(name, np.stack(probs), ks, ps, None, us), np.array(intended), n_top


# --------------------------------------------------------------------------- c. neighbouring floats
def family_c(vocab: int, seed=0) -> Case:
    """Clusters p, nextafter(p), nextafter(nextafter(p)) ... of 300 members (inside one level-2 digit: the top 22
    bits are shared) and 3000 members (three level-1 digits under one level-0 digit), ids in random order; the cut
    falls inside the cluster by top_k, by top_p and by min_p; with two larger tokens above the cluster and without
    (then every kept token shares one level-0 digit)."""
    r = np.random.default_rng(_seed("neigh", vocab, seed))
    probs, ks, ps, ms, us = [], [], [], [], []
    for size in (300, 3000):
        assert vocab >= size + 16
        for with_tops in (True, False):
            base = np.float32(2.0 ** -13).view(np.uint32) + np.uint32(100)      # low 10 bits: 100 .. 399 for 300
            cluster = (base + np.arange(size, dtype=np.uint32)).view(np.float32)
            perm = r.permutation(vocab)
            row = np.zeros(vocab, dtype=np.float32)
            row[perm[:size]] = cluster
            n_top = 2 if with_tops else 0
            row[perm[size:size + n_top]] = [0.25, 0.125][:n_top]
            row[perm[size + n_top:]] = r.random(vocab - size - n_top, dtype=np.float32) * np.float32(1e-9)
            ranked = np.sort(cluster)[::-1]
            mass = np.cumsum(osamp.fx(ranked), dtype=np.uint64)
            top_mass = int(osamp.fx(row[perm[size:size + n_top]]).sum(dtype=np.uint64))
            pmax = row.max()
            for j in (1, size // 3, size // 2 + 7, size - 1):                  # cluster members kept
                for mode in ("k", "p", "minp"):
                    k, p, mp = K_ALL, 1.0, 0.0
                    if mode == "k":
                        k = n_top + j
                    elif mode == "p":
                        p = np.float32((top_mass + int(mass[j - 1])) / osamp.FX_ONE)
                    else:
                        mp = np.float32(ranked[j - 1]) / pmax
                    probs.append(row), ks.append(k), ps.append(p), ms.append(mp), us.append(r.random())
    return Case(f"c_neighbours_v{vocab}", np.stack(probs), ks, ps, ms, us)


# --------------------------------------------------------------------------- d. zeros, denormals, bad entries
def overfull_rows(vocab: int, rows: int, seed=0) -> np.ndarray:
    """fp32 softmax rows whose fx sum exceeds fx(1.0)."""
    g = torch.Generator().manual_seed(_seed("overfull", vocab, seed))
    out = []
    for _ in range(64):
        p = torch.softmax(torch.randn(vocab, generator=g), dim=-1).numpy()
        if int(osamp.fx(p).sum(dtype=np.uint64)) > int(osamp.FX_ONE):
            out.append(p)
            if len(out) == rows:
                break
    assert out, "no fp32 softmax row with an fx sum above fx(1.0) among 64 draws"
    return np.stack(out)


def family_d(vocab: int, with_minp: bool, seed=0) -> Case:
    r = np.random.default_rng(_seed("zeros", vocab, seed))
    probs, ks, ps, ms, us = [], [], [], [], []

    def add(row, k=K_ALL, p=1.0, m=0.0, u=None):
        probs.append(np.asarray(row, dtype=np.float32)), ks.append(k), ps.append(p), ms.append(m)
        us.append(r.random() if u is None else u)

    def sparse(density):
        row = np.zeros(vocab, dtype=np.float32)
        n = max(1, int(vocab * density))
        idx = r.permutation(vocab)[:n]
        v = r.random(n, dtype=np.float32) + np.float32(1e-3)
        row[idx] = v / v.sum(dtype=np.float32)
        return row, n

    denorm = lambda n: (r.integers(1, 1 << 22, n).astype(np.uint32)).view(np.float32)   # fp32 denormals: fx = 0
    row, n = sparse(0.1)
    for k, p, m in ((max(n // 2, 1), 1.0, 0.0), (n, 1.0, 0.0), (n + 1, 1.0, 0.0), (min(n + 37, vocab), 1.0, 0.0),
                    (K_ALL, 1.0, 0.0), (K_ALL, 0.9, 0.0), (K_ALL, 1.0, 0.01), (K_ALL, ONE_BELOW, 1e-7)):
        add(row, k, p, m)
    # denormals: rank above the zeros, carry no mass
    row2 = row.copy()
    zeros = np.flatnonzero(row2 == 0)
    nd = max(1, len(zeros) // 3)
    row2[zeros[:nd]] = denorm(nd)
    for k, p, m in ((n + nd // 2, 1.0, 0.0), (n + nd, 1.0, 0.0), (min(n + nd + 1, vocab), 1.0, 0.0), (n + 1, 0.5, 0.0),
                    (K_ALL, 1.0, 0.0), (K_ALL, 1.0, 1e-7), (K_ALL, 0.999, 0.01)):
        add(row2, k, p, m)
    # bad entries: NaN, negative, -0.0, -inf rank as zero and carry no mass
    row3 = row2.copy()
    bad = r.permutation(vocab)[:max(1, min(9, vocab // 4))]
    row3[bad] = np.resize(np.array([np.nan, -0.25, -0.0, -np.inf, -1e-40], dtype=np.float32), len(bad))
    for k, p, m in ((K_ALL, 1.0, 0.0), (vocab, 1.0, 0.0), (max(vocab - 1, 1), 1.0, 0.0), (max(n // 2, 1), 1.0, 0.0),
                    (K_ALL, 0.7, 0.0), (K_ALL, 1.0, 0.02)):
        add(row3, k, p, m)
    add(np.full(vocab, np.nan, dtype=np.float32))                                  # no mass at all: token 0
    add(np.zeros(vocab), 5, 0.9)
    add(np.zeros(vocab))
    add(denorm(vocab))                                                             # positive rank, zero mass: token 0
    add(denorm(vocab), 3, 0.5, 0.5)
    for hot in (0, vocab // 2, vocab - 1):
        one = np.zeros(vocab, dtype=np.float32)
        one[hot] = 1.0
        add(one, 5, 0.9, 0.0)
        add(one, K_ALL, 1.0, 1.0, u=ONE_BELOW)
    if vocab >= 1024:
        for o in overfull_rows(vocab, 3, seed):
            add(o, K_ALL, 1.0, 0.0)
            add(o, K_ALL, 1.0, 0.0, u=ONE_BELOW)
    # exact_boundary_zero_mass_tail: the kept mass equals fx(top_p) exactly and every token below carries no mass, in
    # several patterns (denormals of more than one level-0 digit, then zeros).  Their exclusive mass == fx(top_p), so
    # all of them are kept; a scan that lets a digit fail at '>=' stops at the largest denormal instead.
    for heads, p in (((1.0,), 1.0), ((0.5, 0.5), 1.0), ((0.5, 0.25), 0.75), ((0.5, 0.25, 0.125), 0.875)):
        nt = max(3, vocab // 4)
        perm = r.permutation(vocab)
        tail = np.zeros(vocab, dtype=np.float32)
        pats = r.integers(1, 1 << 23, nt).astype(np.uint32)
        pats[:3] = (1, (1 << 21) + 5, (3 << 21) + 7)
        tail[perm[:nt]] = pats.view(np.float32)
        tail[perm[nt:nt + len(heads)]] = heads
        add(tail, K_ALL, p, 0.0)
        add(tail, K_ALL, p, 0.0, u=ONE_BELOW)
        add(tail, len(heads) + nt // 2, p, 0.0)
        add(tail, K_ALL, p, 1e-7)
    ms = np.array(ms, dtype=np.float32)
    return Case(f"d_zeros_{'minp' if with_minp else 'nominp'}_v{vocab}", np.stack(probs), ks, ps,
                ms if with_minp else None, us)


# --------------------------------------------------------------------------- f. parameter edges
def family_f(vocab: int, seed=0):
    """The cross product of the edge values over eight model-shaped rows, then the same rows with each parameter
    array absent (a NULL pointer), one at a time and all together."""
    base = model_rows(vocab, 8, ("edges", seed))
    top_ks = [0, 1, vocab - 1, vocab, vocab + 1, 2 ** 31 - 1, -1, -(2 ** 31)]
    top_ps = [np.float32(1e-9), ONE_BELOW, np.float32(1.0)]
    min_ps = [np.float32(0.0), np.float32(1e-7), np.float32(1.0)]
    unis = [np.float32(0.0), ONE_BELOW, np.float32(1.0)]
    rows, ks, ps, ms, us = [], [], [], [], []
    i = 0
    for k in top_ks:
        for p in top_ps:
            for m in min_ps:
                for u in unis:
                    rows.append(base[i % 8]), ks.append(k), ps.append(p), ms.append(m), us.append(u)
                    i += 1
    full = Case(f"f_edges_v{vocab}", np.stack(rows), ks, ps, ms, us)
    cases = [full]
    sub = slice(0, None, 5)                                        # every fifth row of the product: 44 rows
    for name, (hk, hp, hm) in (("no_top_ks", (0, 1, 1)), ("no_top_ps", (1, 0, 1)), ("no_min_ps", (1, 1, 0)),
                               ("no_filters", (0, 0, 0))):
        cases.append(Case(f"f_edges_{name}_v{vocab}", full.probs[sub], full.top_ks[sub] if hk else None,
                          full.top_ps[sub] if hp else None, full.min_ps[sub] if hm else None, full.uniform[sub]))
    return cases


# --------------------------------------------------------------------------- g. position independence
def family_g(vocab: int, batches=(1, 257, 1024), pool_rows: int = 12, seed=0):
    """-> (cases, probe positions per case).  One probe (row, parameters, uniform) at batch index 0, in the middle
    and at the end of batches whose other rows are drawn, in a different order every time, from a pool."""
    pool = family_a(vocab, pool_rows, ("pool", seed))
    probe = 3                                                      # pool row 3: top_k, top_p and min_p all set
    r = np.random.default_rng(_seed("position", vocab, seed))
    cases, positions = [], []
    for bs in batches:
        for where in sorted({0, bs // 2, bs - 1}):
            pick = r.integers(0, pool_rows, bs)
            pick[where] = probe
            cases.append(Case(f"g_position_v{vocab}_bs{bs}_at{where}", pool.probs[pick], pool.top_ks[pick],
                              pool.top_ps[pick], pool.min_ps[pick], pool.uniform[pick]))
            positions.append(where)
    return cases, positions


# --------------------------------------------------------------------------- softmax inputs
def softmax_logits(vocab: int, rows: int, seed=0):
    """bf16-valued logits up to +-60 and temperatures over 0.05 .. 4."""
    g = torch.Generator().manual_seed(_seed("softmax", vocab, seed))
    scale = torch.tensor([1.0, 4.0, 10.0, 20.0] * ((rows + 3) // 4))[:rows].view(-1, 1)
    logits = (torch.randn(rows, vocab, generator=g) * scale).clamp(-60, 60)
    logits[0, 0], logits[0, -1] = 60.0, -60.0
    logits = logits.to(torch.bfloat16).float()
    temps = torch.tensor([0.05, 0.1, 0.3, 0.7, 1.0, 1.7, 2.5, 4.0] * ((rows + 7) // 8))[:rows]
    return logits, temps


def softmax_float64(logits: torch.Tensor, temps: torch.Tensor) -> torch.Tensor:
    """softmax in float64 of the fp32 quotient logits / T (the kernel divides in fp32), rounded to fp32."""
    z = (logits.float() / temps.float().view(-1, 1)).double()
    return torch.softmax(z, dim=-1).float()
