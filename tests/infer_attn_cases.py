"""Cases for the inference attention kernels - attn_decode_kernel and its combine launch (csrc/decode.hip, through
llx.kernels.attn_decode and the C entry llx_attn_decode), attn_dense_fwd_kernel (csrc/attn_dense.hip) and attn_mask_fwd_kernel, the
prefill route (csrc/attn_fwd.hip, csrc/attn_fwd_body.h): one case per class of every axis their launchers distinguish, two operand
families on which softmax attention has exactly one right answer, the float64 reference that computes it, and planted faults in an
emulation of the decode kernel's split walk.  tests/test_infer_attn_cases.py checks all of this on the CPU,
tests/test_infer_attn_exact_gpu.py runs the table on the GPU with torch.equal (selection) and integer equality (census) as the bars.

Selection ("sel"): which q, K, V and o addresses are used.
  Key k of cache (b, kvh) carries the 14-bit code of k XOR salt(b, kvh) in dims 0..13 as +-32 (bit set: +32), Gaussian noise in dims
  14..127; the salts differ for every (b, kvh).  Query row (b, h, m) carries the code of its target key, zeros in dims 14..127; its mask
  row allows the target.  A key at Hamming distance j from the target scores 1024 (14 - 2 j): integers, exact in fp32 whatever the
  order of the sum, and the target leads by 2048 / sqrt(128) = 181.02 nats = 261.2 in log2 units.  exp(-181) and exp2(-261) are 0 in
  fp32 (the smallest denormal is 2^-149), so every other key has weight 0, the target's weight is exp2(0) = 1, the row sum is 1, every
  partial without the target merges with factor 0 and the output row is V[b, kvh, target], bit for bit.
  attn_mask_fwd_kernel scales inside an fma: p = exp2(fma(s, c, -fl(s c))) = 1 +- 4e-5, not 1.  But P goes to bf16 before P.V
  (bf16(1 +- 4e-5) = 1, so O = V exactly), and O / l = V (1 -+ 4e-5) rounds back to the bf16 value V (half an ulp is 2^-9 relative).  The
  deferred base of that kernel never goes stale here: two scores differ by 0 or by at least 261, the base moves at a difference of 8.
  So torch.equal is the bar for all three kernels; no one-ulp fallback is needed.

Census ("cen0", "cen1"): which keys every row attended, each how often.
  q = 0, K finite garbage (9984 among it): every score is 0, every allowed key has weight exp(0) = 1.  V is one-hot: plane 0 has
  V[k, d] = 1 iff k % 128 == d, plane 1 iff (k // 128) % 128 == d; one launch each, together they name every key below 16384.  All sums
  are small integers (exact in fp32 in any order), the output is count_d / count rounded to fp32 (the dense and prefill kernels
  multiply by fl(1 / count): two more roundings of 2^-24) and once to bf16: relative error < 2^-8, so round(o count) == count_d while
  count_d <= 128 < 2^7, which holds for any mask at Skv <= 16384 and is asserted by `build`.  A key left out, counted twice or read
  through another row's mask byte changes an integer: with the key's own count going from c to c -+ 1 and the row's from N to N -+ 1
  the output decodes to c -+ 1 +- (c -+ 1) / (N -+ 1), which rounds back to c only where the key's dim holds half of the row's keys.
  Plane 0 spreads the keys of a row over 128 dims (at most ceil(Skv / 128) each), so it sees every single key of a row with three
  keys or more; plane 1 holds up to 128 keys per dim and is there to tell the keys of a dim of plane 0 apart.
A row without any allowed key is NaN in both families (SDPA's softmax of an all -inf row); its neighbours stay exact.

Dispatch, restated.
  attn_decode: rows = G M query rows per kv head share one read of K / V.  Instances <ROWS, DEC_KPG>: rows <= 4 -> <4, 4> with 16
  partials in LDS (one per lane group), <= 8 -> <8, 2>, <= 16 -> <16, 1>, both with 4 (one per wave); more rows are rejected.  Row r of
  an instance is (head min(r / M, G - 1), token r % M); with a mask shared by the heads (head stride 0: [M, Skv] and [B, 1, M, Skv]) the
  mask byte of row r < M is token min(r, M - 1)'s, expanded to the heads; a per-head mask is read per row and rows r / M >= G are dead.
  The wrapper's nsplit = max(1, min(ceil(Skv / 32), ceil(512 / (B KVH)), 128)); the C entry takes 1..1024.  With ext = min(*extent, Skv)
  (Skv without an extent): span = round_up_16(ceil(ext / nsplit)), split i owns keys [i span, min(ext, (i + 1) span)) - empty from
  ceil(ext / span) on.  Inside a split wave w starts at k_lo + 4 KPG w and advances by 16 KPG; in a step lane group g, load j reads key
  k0 + 4 j + g, clamped to Skv - 1 and masked from k_hi on.  The two register sets swap from the third step on.
  attn_dense_fwd: one wave per (b, h, query row), 64-key chunks; a chunk whose keys are all masked for the row is skipped whole.
  attn_mask_fwd: 128-row blocks x 64-key tiles with classes 0 (nothing allowed, skipped), 1 (partly masked, tests the mask bytes),
  2 (all 128 x 64 allowed; rows past Sq do not count, a ragged last tile is never 2).
"""
import functools
import math
import zlib
from dataclasses import dataclass

import torch

from oracle import ref as O

BF16 = torch.bfloat16
HD = 128
SENTINEL = -(2.0 ** 100)  # exact in bf16, no output of these cases equals it
FAMILIES = ("sel", "cen0", "cen1")
CODE_BITS = 14
ROW_CLASSES = ((1, 1), (3, 1), (4, 1), (1, 4), (2, 2), (5, 1), (2, 3), (3, 2), (8, 1), (1, 8), (2, 4), (3, 3), (5, 3), (2, 5), (4, 4),
               (16, 1), (1, 16))
FORMS = ("shared", "batch", "head")


# ------------------------------------------------------------------------------------------------------------------------ dispatch
def decode_instance(G: int, M: int):
    """(ROWS, DEC_KPG, NPART) of attn_decode_kernel for G heads per group and M tokens, None where llx_attn_decode rejects."""
    rows = G * M
    if rows > 16:
        return None
    return (4, 4, 16) if rows <= 4 else ((8, 2, 4) if rows <= 8 else (16, 1, 4))


def decode_nsplit(B: int, KVH: int, Skv: int) -> int:
    return max(1, min(-(-Skv // 32), -(-512 // (B * KVH)), 128))


def nsplit_term(B: int, KVH: int, Skv: int) -> str:
    """Which term of the wrapper's formula decides: keys | wgs | cap (ties named together)."""
    a, b, n = -(-Skv // 32), -(-512 // (B * KVH)), decode_nsplit(B, KVH, Skv)
    return "+".join(t for t, v in (("keys", a), ("wgs", b), ("cap", 128)) if v == n)


def decode_span(ext: int, nsplit: int) -> int:
    return ((ext + nsplit - 1) // nsplit + 15) & ~15


@dataclass(frozen=True)
class Plan:
    rows: int
    inst: tuple      # (ROWS, KPG, NPART)
    nsplit: int
    ext: int
    span: int
    splits: tuple    # (k_lo, k_hi) of every split; an empty one is (k_lo, k_lo)

    @property
    def kpg(self):
        return self.inst[1]

    @property
    def live(self):
        return [i for i, (lo, hi) in enumerate(self.splits) if hi > lo]

    @property
    def empty(self):
        return self.nsplit - len(self.live)

    def steps(self, split: int, wave: int) -> int:
        lo, hi = self.splits[split]
        return len(range(lo + wave * 4 * self.kpg, hi, 16 * self.kpg)) if hi > lo else 0

    @property
    def step_classes(self) -> set:
        """{0, 1, 2, 3}: steps per wave over the live splits, 3 standing for three or more."""
        return {min(3, self.steps(s, w)) for s in self.live for w in range(4)}

    @property
    def ragged(self) -> bool:
        return self.ext % 16 != 0

    def owner(self, key: int) -> tuple:
        """(split, step, wave, load j, lane group) that reads key < ext."""
        s = key // self.span
        off = key - s * self.span
        kstep = 16 * self.kpg
        return s, off // kstep, (off % kstep) // (4 * self.kpg), (off % (4 * self.kpg)) // 4, off % 4


def decode_plan(G: int, M: int, Skv: int, ext: int, nsplit: int) -> Plan:
    ext = min(ext, Skv)
    span = decode_span(ext, nsplit)
    splits = tuple((i * span, max(i * span, min(ext, (i + 1) * span))) for i in range(nsplit))
    return Plan(G * M, decode_instance(G, M), nsplit, ext, span, splits)


def dense_chunks(Skv: int) -> int:
    return -(-Skv // 64)


def tile_classes(mask: torch.Tensor) -> torch.Tensor:
    """uint8 [B, ceil(Sq / 128), ceil(Skv / 64)] of a bool mask [B, Sq, Skv]: what llx_attn_mask_tile_flags computes."""
    B, Sq, Skv = mask.shape
    nqb, nkt = -(-Sq // 128), -(-Skv // 64)
    out = torch.zeros(B, nqb, nkt, dtype=torch.uint8)
    for qb in range(nqb):
        for kt in range(nkt):
            t = mask[:, qb * 128:(qb + 1) * 128, kt * 64:(kt + 1) * 64]
            anyv, allv = t.flatten(1).any(1), t.flatten(1).all(1) & (t.shape[2] == 64)
            out[:, qb, kt] = anyv.to(torch.uint8) + (anyv & allv).to(torch.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    id: str
    kernel: str          # decode | dense | prefill
    B: int
    KVH: int
    G: int
    M: int               # query tokens (decode) / Sq
    Skv: int
    form: str            # shared [M, Skv] | batch [B, 1, M, Skv] | head [B, H, M, Skv] | tiles (prefill: [B | 1, 1, Sq, Skv] by tile class)
    live: int = 0        # keys any row may attend to (0: all Skv); the mask's extent
    nsplit: int = 0      # decode: 0 = the wrapper's; else through the C entry
    nan: bool = False    # one row (shared and batch forms: one token, every head) without any allowed key
    chunk: str = ""      # dense: first | middle | last 64-key chunk masked whole for every row
    shift: int = 0       # prefill: rotation of the tile-class pattern
    pad: int = 0         # prefill: bytes between the mask rows the kernel is given (1, 3: an odd row stride where Skv is even)

    @property
    def H(self):
        return self.KVH * self.G

    @property
    def ext(self):
        return self.live or self.Skv

    def plan(self, use_ext: bool = True) -> Plan:
        ns = self.nsplit or decode_nsplit(self.B, self.KVH, self.Skv)
        return decode_plan(self.G, self.M, self.Skv, self.ext if use_ext else self.Skv, ns)


def _table() -> dict:
    cs = []
    # decode, row classes x mask forms at 200 keys (7 splits of 32, the last one 8 keys: a partly filled group); KVH 1 and 2
    for i, (g, m) in enumerate(ROW_CLASSES):
        for f, form in enumerate(FORMS):
            cs.append(Case(f"dec_g{g}m{m}_{form}", "decode", 2, 1 + (i + f) % 2, g, m, 200, form, nan=(i + f) % 3 == 0 and (form != "shared" or m > 1)))
    # decode, cache lengths: nsplit 1 (<= 32 keys) | 2; mostly empty splits; 128 splits; four splits with three steps per wave
    for j, skv in enumerate((1, 17, 32, 33)):
        for f, (g, m) in enumerate(((4, 1), (2, 3), (3, 3))):
            cs.append(Case(f"dec_s{skv}_g{g}m{m}", "decode", 2, 2, g, m, skv, FORMS[(j + f) % 3]))
    for f, (g, m) in enumerate(((4, 1), (3, 2), (2, 5))):
        cs.append(Case(f"dec_s1000live65_g{g}m{m}", "decode", 2, 2, g, m, 1000, FORMS[f], live=65))
    cs.append(Case("dec_s4101_g4m1", "decode", 1, 2, 4, 1, 4101, "head"))
    cs.append(Case("dec_s4101_g2m3", "decode", 3, 1, 2, 3, 4101, "batch"))
    cs.append(Case("dec_s8197_g2m2", "decode", 2, 2, 2, 2, 8197, "batch", nan=True))
    cs.append(Case("dec_s8197_g16m1", "decode", 1, 1, 16, 1, 8197, "head"))
    cs.append(Case("dec_s8197_g1m3", "decode", 2, 2, 1, 3, 8197, "shared", nan=True))
    for f, (g, m) in enumerate(((2, 2), (2, 3), (3, 3))):  # B KVH = 128: four splits of 144 keys, three to nine steps per wave
        cs.append(Case(f"dec_b16kvh8_g{g}m{m}", "decode", 16, 8, g, m, 520, ("batch", "head", "shared")[f]))
    # decode, the C entry: nsplit 3 (a combine group without a partial), 40 (> ceil(200 / 16) = 13), 1024
    for ns in (3, 40, 1024):
        cs.append(Case(f"abi_rows4_n{ns}", "decode", 2, 2, 2, 2, 200, "head", nsplit=ns, nan=True))
        cs.append(Case(f"abi_rows16_n{ns}", "decode", 1, 1, 16, 1, 200, "shared", nsplit=ns))
    # dense
    for j, skv in enumerate((1, 63, 64, 65, 130)):
        for f, form in enumerate(FORMS):
            cs.append(Case(f"dense_s{skv}_{form}", "dense", 2, 2, (1, 3)[(j + f) % 2], (17, 1)[(j // 2 + f) % 2], skv, form, nan=form == "head"))
    for f, ch in enumerate(("first", "middle", "last")):
        cs.append(Case(f"dense_chunk_{ch}", "dense", 2, 1, (3, 1, 3)[f], 17, 130, FORMS[f], chunk=ch))
    # prefill
    for j, (sq, skv, b) in enumerate(((1, 4, 1), (17, 63, 2), (128, 64, 2), (129, 65, 2), (300, 700, 2), (17, 4300, 1), (300, 4300, 2), (129, 700, 1),
                                      (128, 64, 1), (300, 64, 2), (1, 700, 2), (129, 4, 2))):
        cs.append(Case(f"pre_q{sq}_k{skv}_b{b}", "prefill", b, 2, 1 + j % 2, sq, skv, "tiles", shift=(1, 1, 2, 4, 5, 6, 7, 8, 2, 10, 11, 12)[j], pad=(0, 3, 1)[j % 3]))
    return {c.id: c for c in cs}


CASES = _table()


def cases_of(kernel: str) -> list:
    return [c for c in CASES.values() if c.kernel == kernel]


# ------------------------------------------------------------------------------------------------------------------------ operands
def _bits(name: str, shape) -> torch.Tensor:
    return O.randint(name, shape, 0, 2).bool()


def build_mask(c: Case) -> torch.Tensor:
    """The bool mask in the form the kernel is given: [M, Skv], [B, 1, M, Skv] or [B, H, M, Skv]; False from c.ext on, and the key
    c.ext - 1 allowed for some row, so that the mask's extent is c.ext."""
    B, H, M, S, L = c.B, c.H, c.M, c.Skv, c.ext
    if c.form == "shared":
        m = torch.zeros(M, S, dtype=torch.bool)
        m[:, :L] = _bits(f"ia_m_{c.id}", (M, L))
        m[0, L - 1] = True
        if c.nan and M > 1:
            m[M - 1] = False
    elif c.form == "batch":  # a live range per sequence (left padding, its own length), causal over the call's tokens
        m = torch.zeros(B, 1, M, S, dtype=torch.bool)
        for b in range(B):
            hi = max(1, L - 7 * b)
            lo = min(3 * b, hi - 1)
            for t in range(M):
                m[b, 0, t, lo:max(lo + 1, hi - (M - 1 - t))] = True
        if c.nan:
            m[B - 1, 0, 0] = False
    elif c.form == "head":
        m = torch.zeros(B, H, M, S, dtype=torch.bool)
        m[..., :L] = _bits(f"ia_m_{c.id}", (B, H, M, L))
        m[0, 0, 0, L - 1] = True
        if c.nan:
            m[B - 1, H - 1, M - 1] = False
    else:  # tiles: class (qb + kt + b + shift) % 3 per 128 x 64 tile; a class-2 fill of a ragged tile is class 1 by the rule
        m = torch.zeros(B, 1, M, S, dtype=torch.bool)
        rnd = _bits(f"ia_m_{c.id}", (B, M, S))
        for b in range(B):
            for qb in range(-(-M // 128)):
                for kt in range(-(-S // 64)):
                    cls = (qb + kt + b + c.shift) % 3
                    sl = (b, 0, slice(qb * 128, (qb + 1) * 128), slice(kt * 64, (kt + 1) * 64))
                    if cls == 2:
                        m[sl] = True
                    elif cls == 1:
                        m[sl] = rnd[b, sl[2], sl[3]]
                        m[b, 0, qb * 128, kt * 64] = True
                        if kt * 64 + 1 < S:
                            m[b, 0, qb * 128, kt * 64 + 1] = False
    if c.chunk:
        i = {"first": 0, "middle": 1, "last": dense_chunks(S) - 1}[c.chunk]
        m[..., i * 64:(i + 1) * 64] = False
    return m


def expand_mask(c: Case, m: torch.Tensor) -> torch.Tensor:
    while m.dim() < 4:
        m = m.unsqueeze(0)
    return m.expand(c.B, c.H, c.M, c.Skv)


def mask_extent(m4: torch.Tensor) -> int:
    idx = m4.any(0).any(0).any(0).nonzero()
    return int(idx.max()) + 1 if idx.numel() else 0


def salt(c: Case, b: int, kvh: int) -> int:
    return ((b * c.KVH + kvh) * 2731 + 1) & ((1 << CODE_BITS) - 1)


def _code(x: torch.Tensor) -> torch.Tensor:
    """[..., 14] of +-32 for int64 x."""
    bit = (x.unsqueeze(-1) >> torch.arange(CODE_BITS)) & 1
    return (bit * 64 - 32).float()


def decode_edges(p: Plan) -> list:
    """The keys the plan names: key 0, the first and last key of a split, the last live key, the first key of a partly filled last
    16-key group, and keys read by every wave, lane group and load of the first and the last full split."""
    live = p.live
    if not live:
        return []
    e = [0, p.ext - 1]
    for s in (live[0], live[len(live) // 2], live[-1]):
        e += [p.splits[s][0], p.splits[s][1] - 1]
    if p.ragged:
        e.append(p.ext - p.ext % 16)
    for s in {live[0], live[max(0, len(live) - 2)]}:
        lo, hi = p.splits[s]
        for step in (0, 2):
            for w in range(4):
                for j in range(p.kpg):
                    for g in range(4):
                        k = lo + step * 16 * p.kpg + w * 4 * p.kpg + 4 * j + g
                        if k < hi:
                            e.append(k)
    return list(dict.fromkeys(e))


def _edges_of(c: Case, m4: torch.Tensor):
    """row (b, m) -> the candidate target keys, in order of preference."""
    if c.kernel == "decode":
        e = decode_edges(c.plan(True)) + decode_edges(c.plan(False))
        return lambda b, m: e
    if c.kernel == "dense":
        e = [k for k in (0, 63, 64, 127, 128, c.Skv - 1) if k < c.Skv]
        return lambda b, m: e
    cls = tile_classes(m4[:, 0])
    nkt = cls.shape[2]

    def edges(b, m):
        out = []
        for want in ((1, 2) if m % 2 else (2, 1)):
            ts = [t for t in range(nkt) if cls[b, m // 128, t] == want]
            for t in dict.fromkeys(ts[:1] + ts[len(ts) // 2:len(ts) // 2 + 1] + ts[-1:]):
                out += [t * 64, min(t * 64 + 63, c.Skv - 1), min(t * 64 + 29, c.Skv - 1)]
        return out
    return edges


def pick_targets(c: Case, m4: torch.Tensor) -> torch.Tensor:
    """int64 [B, H, M]: an allowed key for every row, an edge of the plan where the row's mask allows one; -1 for a row without keys."""
    edges = _edges_of(c, m4)
    tgt = torch.full((c.B, c.H, c.M), -1, dtype=torch.int64)
    i = zlib.crc32(c.id.encode()) % 97
    for b in range(c.B):
        for m in range(c.M):
            e = edges(b, m)
            for h in range(c.H):
                row = m4[b, h, m]
                cand = [k for k in e if row[k]]
                if not cand:
                    cand = row.nonzero().flatten().tolist()
                if cand:
                    tgt[b, h, m] = cand[i % len(cand)]
                i += 5
    return tgt


@functools.lru_cache(maxsize=6)
def build(cid: str, fam: str) -> dict:
    """q [B, H, M, 128], k / v [B, KVH, Skv, 128] (bf16), mask (the kernel's form), mask4 (expanded), ext, and the expectation:
    sel: want bf16 [B, H, M, 128] = V[target] (NaN rows where no key is allowed), tgt; census: count int64 [B, H, M], count_d [.., 128]."""
    c = CASES[cid]
    B, H, KVH, G, M, S = c.B, c.H, c.KVH, c.G, c.M, c.Skv
    assert S <= 1 << CODE_BITS and fam in FAMILIES
    mask = build_mask(c)
    m4 = expand_mask(c, mask)
    d = {"case": c, "fam": fam, "mask": mask, "mask4": m4, "ext": mask_extent(m4)}
    if c.kernel == "decode":
        assert d["ext"] == c.ext, (cid, d["ext"])
    keys = torch.arange(S)
    if fam == "sel":
        tgt = pick_targets(c, m4)
        k = O.randn(f"ia_k_{cid}", (B, KVH, S, HD), 1.0)
        for b in range(B):
            for kv in range(KVH):
                k[b, kv, :, :CODE_BITS] = _code(keys ^ salt(c, b, kv))
        salts = torch.tensor([[salt(c, b, h // G) for h in range(H)] for b in range(B)])
        q = torch.zeros(B, H, M, HD)
        q[..., :CODE_BITS] = _code(tgt.clamp_min(0) ^ salts[:, :, None])
        v = O.randn(f"ia_v_{cid}", (B, KVH, S, HD), 1.0).to(BF16)
        want = v.repeat_interleave(G, 1).gather(2, tgt.clamp_min(0)[..., None].expand(B, H, M, HD)).clone()
        want[tgt < 0] = float("nan")
        assert (want.float() != SENTINEL).all() and (m4.gather(3, tgt.clamp_min(0)[..., None])[..., 0] | (tgt < 0)).all()
        d.update(q=q.to(BF16), k=k.to(BF16), v=v, tgt=tgt, want=want)
    else:
        k = O.randn(f"ia_kc_{cid}", (1, 1, S, HD), 50.0).expand(B, KVH, S, HD).clone()
        k.view(-1)[::37] = 1e4
        idx = keys % HD if fam == "cen0" else (keys // HD) % HD
        v1 = torch.zeros(S, HD)
        v1[keys, idx] = 1.0
        count = m4.sum(-1)
        count_d = (m4.reshape(-1, S).double() @ v1.double()).reshape(B, H, M, HD).round().long()
        assert int(count_d.max()) <= 128 and torch.equal(count_d.sum(-1), count)
        d.update(q=torch.zeros(B, H, M, HD, dtype=BF16), k=k.to(BF16), v=v1.to(BF16).expand(B, KVH, S, HD).contiguous(), count=count, count_d=count_d)
    return d


# ------------------------------------------------------------------------------------------------------------------------ references
def rbf(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(BF16)


def weighted_sdpa64(q, k, v, W, extra=None) -> torch.Tensor:
    """float64 softmax attention in which row (b, h, m) counts key k W[b, h, m, k] times (W = the bool mask: SDPA itself); `extra`
    partials with row sum 1 and output 1 in every dim are merged in at factor 1 (the `empty_factor1` fault).  0 / 0 = NaN for a row
    without keys, as softmax of an all -inf row.  [B, H, M, 128] float64."""
    B, H, M, _ = q.shape
    KVH, S = k.shape[1], k.shape[2]
    G = H // KVH
    qg = q.double().reshape(B, KVH, G * M, HD)
    s = torch.einsum("bgrd,bgkd->bgrk", qg, k.double()) / math.sqrt(HD)
    Wg = W.reshape(B, KVH, G * M, S).double()
    s = s.masked_fill(Wg == 0, float("-inf"))
    smax = s.max(-1, keepdim=True).values
    smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
    p = Wg * torch.exp(s - smax)
    num = torch.einsum("bgrk,bgkd->bgrd", p, v.double())
    den = p.sum(-1, keepdim=True)
    if extra is not None:
        ex = extra.reshape(B, KVH, G * M, 1).double()
        num, den = num + ex, den + ex
    return (num / den).reshape(B, H, M, HD)


def sdpa64(d: dict) -> torch.Tensor:
    return weighted_sdpa64(d["q"], d["k"], d["v"], d["mask4"])


def sel_ok(o: torch.Tensor, d: dict) -> bool:
    """o bf16 [B, H, M, 128] against V[target]: bit for bit, NaN where the row has no key."""
    w = d["want"]
    nan = torch.isnan(w.float())
    return bool(torch.equal(torch.isnan(o.float()), nan) and torch.equal(o.float().masked_fill(nan, 0), w.float().masked_fill(nan, 0)))


def census_decode(o: torch.Tensor, d: dict) -> torch.Tensor:
    """int64 [B, H, M, 128]: the counts an output names, round(o count); -1 in rows that must be (and are) NaN, -2 where NaN is wrong."""
    cnt = d["count"][..., None]
    got = torch.round(o.double() * cnt)
    nan = torch.isnan(o.float())
    got = torch.where(nan, torch.where(cnt == 0, -1.0, -2.0).expand_as(got).double(), got)
    return got.long()


def census_ok(o: torch.Tensor, d: dict) -> bool:
    want = torch.where((d["count"] == 0)[..., None], torch.full_like(d["count_d"], -1), d["count_d"])
    return bool(torch.equal(census_decode(o, d), want))


def family_ok(o: torch.Tensor, d: dict) -> bool:
    return sel_ok(o, d) if d["fam"] == "sel" else census_ok(o, d)


# ------------------------------------------------------------------------------------------------------------------------ the split walk
# drop_last / double_first hit every split, as an off-by-one in k_hi or an inclusive bound would; the *_one forms hit a single split
# (the first one from the middle on whose key some row attends), as a fault in one workgroup's bounds or one partial's slot would
FAULTS = ("drop_last", "double_first", "drop_last_one", "double_first_one", "span_round_down", "clamp_row", "head_minus1", "batch0", "empty_factor1")


def walk_counts(c: Case, use_ext: bool, fault: str = "", only: int = -1) -> torch.Tensor:
    """int64 [Skv]: how often the split walk of attn_decode_kernel hands every key to the softmax - splits, waves, steps, loads and lane
    groups as the kernel runs them (1 below ext and 0 from there on, when nothing is wrong).  only: the split drop_last / double_first
    are confined to (-1: every split)."""
    p = c.plan(use_ext)
    span = p.span
    if fault == "span_round_down":
        span = ((p.ext + p.nsplit - 1) // p.nsplit) & ~15
    if fault == "span_ceil_only":  # not a fault: the walk does not need the multiple of 16 (tests/test_infer_attn_cases.py says so)
        span = (p.ext + p.nsplit - 1) // p.nsplit
    cnt = torch.zeros(c.Skv, dtype=torch.int64)
    kstep = 16 * p.kpg
    for split in range(p.nsplit):
        k_lo = split * span
        k_hi = min(p.ext, k_lo + span)
        here = only < 0 or only == split
        stop = k_hi - 1 if fault == "drop_last" and here else k_hi
        for wave in range(4):
            k0 = k_lo + wave * 4 * p.kpg
            while k0 < k_hi:
                for j in range(p.kpg):
                    for grp in range(4):
                        key = k0 + 4 * j + grp
                        if key < stop:
                            cnt[min(key, c.Skv - 1)] += 1
                k0 += kstep
        if fault == "double_first" and here and k_lo < k_hi:
            cnt[k_lo] += 1
    return cnt


def emulate(c: Case, mask4: torch.Tensor, use_ext: bool = True, fault: str = "") -> tuple:
    """(W int64 [B, H, M, Skv], extra int64 [B, H, M]): how often row (b, h, m) counts key k - the mask byte the kernel's indexing reads
    times the walk's count - and how many empty splits are merged at factor 1 instead of 0.  A partial of an empty split is (m, l, o)
    = (-inf, 0, 0) in the kernel, which no factor can show; the emulation gives it l = 1 and o = 1, what a factor of 1 would let through
    if the slot held anything."""
    B, H, M, G = c.B, c.H, c.M, c.G
    eff = mask4
    if fault == "clamp_row" and c.form in ("shared", "batch") and M > 1:  # min(r, M - 2) for min(r, M - 1)
        eff = mask4[:, :, [min(m, M - 2) for m in range(M)]]
    if fault == "head_minus1" and c.form == "head":
        eff = mask4[:, [h // G * G + max(h % G - 1, 0) for h in range(H)]]
    if fault == "batch0" and c.form in ("batch", "head"):
        eff = mask4[:1].expand_as(mask4)
    only = -1
    if fault.endswith("_one"):
        fault = fault[:-4]
        p = c.plan(use_ext)
        seen = mask4.any(0).any(0).any(0)
        live = p.live[len(p.live) // 2:] + p.live[:len(p.live) // 2]
        only = next(s for s in live if seen[p.splits[s][0] if fault == "double_first" else p.splits[s][1] - 1])
    W = eff.long() * walk_counts(c, use_ext, fault, only)
    extra = torch.zeros(B, H, M, dtype=torch.int64)
    if fault == "empty_factor1":
        extra += c.plan(use_ext).empty
    return W, extra


def fault_applies(c: Case, fault: str, use_ext: bool = True) -> bool:
    """Whether the case is aimed at the fault's class."""
    p = c.plan(use_ext)
    return {"drop_last": True, "double_first": p.ext > 1,  # (twice the only key is still the only key)
            "drop_last_one": True, "double_first_one": p.ext > 1,
            "span_round_down": p.nsplit * (((p.ext + p.nsplit - 1) // p.nsplit) & ~15) < p.ext,
            # (the mask rows of two tokens, heads or sequences are sure to differ from 17 keys on)
            "clamp_row": c.form in ("shared", "batch") and c.M > 1 and c.ext >= 17, "head_minus1": c.form == "head" and c.G > 1 and c.ext >= 17,
            "batch0": c.form in ("batch", "head") and c.B > 1 and c.ext >= 17, "empty_factor1": p.empty > 0}[fault]


def old_bar_accepts(got: torch.Tensor, want: torch.Tensor) -> bool:
    """The bar of test_attn_decode_against_oracle_sdpa: max error within 0.02 of the largest reference magnitude (NaN rows must agree)."""
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    g, w = got.masked_fill(nan, 0), want.masked_fill(nan, 0)
    return float((g - w).abs().max()) <= 0.02 * float(w.abs().max()) + 1e-6
