"""Cases for the training attention kernels - llx_attn_fwd / llx_attn_fwd_dropout (csrc/attn_fwd.hip, attn_fwd_body.h) and the backward
of csrc/attn_bwd.hip: attn_bwd_dq_kernel, attn_bwd_dkv3_kernel, attn_dkv_reduce_kernel (route (b), also from a dense mask through
llx_attn_mask_bwd and in the dropout builds), attn_bwd_delta_kernel, the DS build of dK/dV and attn_bwd_dq2_kernel (route (a)).  The
launchers' walks restated, one case per class they distinguish, operand families on which every gradient has exactly one right value,
and an emulation of the walks with planted faults.  tests/test_train_attn_cases.py checks all of it on the CPU,
tests/test_train_attn_exact_gpu.py runs the table on the GPU with torch.equal / integer equality as the only bars.

The backward is a function of (q, k, v, o, do, lse); the families hand it an o and an lse of their own.

Census ("cenA0", "cenA1", "cenB0", "cenB1"): which rows reached which keys, with which lse and delta.
  Q is non-zero in one half of the 128 dims, K in the other (A: Q in 0..63, K in 64..127; B: swapped), so every score is exactly 0.
  Both are one-hot codes of the position: plane 0 codes index % 64, plane 1 (index // 64) % 64, rotated by a salt of (b, head) or
  (b, kv head).  lse[b, h, q] = L, a hashed integer in 0..3: P = exp2(fma(0, c, -L)) = 2^-L exactly, 0 where masked.  dO is one-hot (value
  1) at dim (q + 37 h + 11 b) % 128, V holds hashed integers in -3..3, O in -1..1: dP = V[k, dim(q)], delta = O[q, dim(q)], and
  dS = 2^-L (dP - delta) is m 2^-L with |m| <= 4 (|m| <= 7 under dropout at p = 1/2, where dP doubles) - at most three significant bits,
  exact in bf16.  Every accumulated sum is a multiple of 2^-3 below 2^24 2^-3: exact in fp32 in any order.  Then
    dV = bf16(sum 2^-L dO), dK = bf16(fl32(scale) . sum dS Q) over the heads of the group, dQ = bf16(fl32(scale) . sum dS K),
  the product with the scale in fp32 as the kernels do it.  dV names the rows that reached each key, dQ / dK the keys and rows of each
  product and the delta and lse they were weighted with.
Selection ("sel"): the operand reads of the score product and the real magnitude of lse.
  Key k carries the 14-bit code of k XOR salt(b, kvh) in dims 0..13 as +-32 (tests/infer_attn_cases.py), noise elsewhere; row (b, h, q)
  carries m / 32 times the code of a target its mask allows, m = 32 or 24 by a hash of the row.  The target scores 14 . 32 m, every other
  key at least 64 m less: 195 log2 units at m = 24, and exp2(-195) = 0 in fp32.  lse = fl32(score . scale_log2), what the forward of the
  same operands writes (tests/test_train_attn_cases.py checks it against sdpa64): P = 1 +- 1e-4 at the target, bf16(P) = 1; with the
  lse of a neighbouring row of the other magnitude P is 0 or inf.  O is given as 0, so delta = 0 (with the true O = V[target] the score
  gradient of a one-hot row vanishes and would test nothing).  V holds integers in -3..3, dO integers in -2..2 in 8 hashed dims:
  dP = dO . V[t] is an integer below 64, dS = bf16(P dP) = dP, dV[t] = sum of the dO of the rows aimed at t, dQ = bf16(scale . dP K[t]) a
  single product, dK[t] = bf16(scale . sum dP Q).
Forward: the sel / cen0 / cen1 families of tests/infer_attn_cases.py (their code, salts, reference and decoders are imported) in the
  layout of llx_attn_fwd; lse against float64 (attn_cases.LSE_REL) and, on census rows, round(exp2(lse)) == count.
Dropout: threshold 32768, so a kept element is scaled by exactly 2; the keep bytes come from kernels.attn_dropout_keep.
Rope: tables whose (cos, sin) are (1, 0), (0, 1), (-1, 0) or (0, -1) by a hash of (position, pair): the epilogue is a signed permutation.
Rows without a key (left padding): lse = -inf; their dq row is not compared, everything else must equal the expectation in which
  they contribute nothing.

Dispatch, restated.
  llx_attn_fwd: workgroups of 256 rows (8 waves x 32), 64-key tiles, causal (kt_end by index arithmetic) or rule (tile flags per 128-row
  block: 0 skip, 1 test the rule, 2 no test; kept 64 tiles per register, reloaded from tile 64 on).
  attn_bwd_dq_kernel: 128-row blocks, 64-key tiles, next_tile skips class 0; causal kt_end = min(nkt, ceil((128 qb + 128) / 64)), class 2
  iff 64 t + 63 <= 128 qb.  A ragged last key tile clamps its keys to S - 1 and masks them (rule: kk < S; mask: the ragged word is read
  at S - 4 and shifted).  Stores 16 bytes wide iff dq and its strides are 16-byte aligned, else 8.
  attn_bwd_dkv3_kernel: 128-key blocks, wave w owns keys 32 w .. of tile my_kt = 2 kblk + (w >> 1), nothing to do where my_kt >= nkt;
  64-row query tiles from qt_first = 2 kblk (causal) or 0; class by 64 x 64 index arithmetic (causal) or the 128 x 64 flag of (qt >> 1,
  my_kt), 64 query blocks per register (reloaded from row 8192 on); class 2 is demoted to 1 on the ragged last query tile, whose rows
  are clamped to S - 1 and masked by qi < S.  One fp32 partial per head; attn_dkv_reduce_kernel sums the G of a group.
  Route (a): attn_bwd_delta_kernel, the DS build of dK/dV storing bf16 dS^T in [Sp, Sp] tiles (Sp = round_up(S, 256)),
  attn_bwd_dq2_kernel summing K^T dS^T over the stored tiles; with flags and more than 128 key tiles llx_attn_bwd falls back to (b).
"""
import functools
import math
import zlib
from dataclasses import dataclass

import torch

from oracle import ref as O
from tests import attn_cases as A
from tests import infer_attn_cases as I

BF16 = torch.bfloat16
HD = 128
BQ, BKV, DKV_KEYS, DKV_QT, FWD_ROWS, DQ2_ROWS = 128, 64, 128, 64, 256, 256
SENTINEL = -(2.0 ** 100)
SCALE = 1.0 / math.sqrt(HD)
SCALE32 = torch.tensor(SCALE, dtype=torch.float32)                       # what the C entries receive
SCALE_LOG2_32 = SCALE32 * torch.tensor(1.4426950408889634, dtype=torch.float32)  # a.scale_log2
CEN = ("cenA0", "cenA1", "cenB0", "cenB1")
BWD_FAMILIES = CEN + ("sel",)
FWD_FAMILIES = I.FAMILIES
DROP_T = 32768
RULE, DENSE = ("doc", "prefix", "docprefix"), ("window", "blocks", "deadblock", "leftpad", "eqcausal")


# ------------------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    id: str
    S: int
    B: int
    KVH: int
    G: int
    mask: str            # causal | doc | prefix | docprefix | window | blocks | deadblock | leftpad | eqcausal
    form: str = ""       # dense masks: ss [S, S] | b1ss [B, 1, S, S] | strided (rows of a wider buffer)
    route_a: bool = False
    dropout: bool = False
    rope: bool = False
    narrow: bool = False  # dq (and the forward's o) at an 8-byte, not 16-byte, aligned address

    @property
    def H(self):
        return self.KVH * self.G

    @property
    def mode(self):
        return "causal" if self.mask == "causal" else ("rule" if self.mask in RULE else "mask")

    @property
    def long(self):
        return self.S > 1024


def _table() -> dict:
    c = Case
    cs = [
        c("causal_s1", 1, 1, 1, 1, "causal", route_a=True, rope=True),
        c("causal_s31", 31, 2, 2, 2, "causal", dropout=True),
        c("causal_s64", 64, 1, 3, 1, "causal", route_a=True, narrow=True),
        c("causal_s129", 129, 2, 1, 4, "causal", rope=True, narrow=True),
        c("causal_s197", 197, 3, 1, 2, "causal", route_a=True, dropout=True),
        c("causal_s257", 257, 1, 1, 8, "causal"),
        c("causal_s449", 449, 2, 2, 1, "causal", route_a=True, rope=True),
        c("causal_s705", 705, 1, 1, 2, "causal", dropout=True, narrow=True),
        c("doc_s5", 5, 2, 1, 2, "doc"),
        c("prefix_s33", 33, 3, 2, 1, "prefix", route_a=True),
        c("docprefix_s63", 63, 2, 1, 4, "docprefix", dropout=True),
        c("doc_s65", 65, 1, 3, 2, "doc", rope=True),
        c("prefix_s127", 127, 2, 2, 2, "prefix", route_a=True, narrow=True),
        c("docprefix_s191", 191, 2, 1, 1, "docprefix", dropout=True, rope=True),
        c("doc_s255", 255, 2, 1, 8, "doc"),
        c("prefix_s320", 320, 3, 1, 2, "prefix", route_a=True),
        c("docprefix_s449", 449, 2, 2, 2, "docprefix", route_a=True, dropout=True),
        c("doc_s705", 705, 2, 1, 2, "doc", rope=True, narrow=True),
        c("prefix_s4160", 4160, 1, 1, 1, "prefix", route_a=True, dropout=True),
        c("docprefix_s8256", 8256, 1, 1, 1, "docprefix", route_a=True),
        c("eqcausal_s4", 4, 2, 1, 2, "eqcausal", "ss"),
        c("window_s5", 5, 2, 2, 1, "window", "b1ss"),
        c("leftpad_s31", 31, 3, 1, 2, "leftpad", "b1ss"),
        c("blocks_s65", 65, 2, 2, 1, "blocks", "strided", rope=True),
        c("window_s129", 129, 1, 1, 4, "window", "ss", narrow=True),
        c("leftpad_s197", 197, 2, 1, 2, "leftpad", "strided"),
        c("blocks_s257", 257, 2, 1, 2, "blocks", "b1ss"),
        c("deadblock_s320", 320, 2, 3, 1, "deadblock", "ss"),
        c("deadblock_s449", 449, 2, 1, 2, "deadblock", "strided"),
        c("blocks_s705", 705, 2, 1, 2, "blocks", "b1ss", rope=True),
        c("eqcausal_s191", 191, 1, 1, 8, "eqcausal", "strided"),
        c("window_s4160", 4160, 1, 1, 1, "window", "ss"),
        c("blocks_s8256", 8256, 1, 1, 1, "blocks", "strided"),
    ]
    return {x.id: x for x in cs}


CASES = _table()
SIZES = (1, 4, 5, 31, 33, 63, 64, 65, 127, 129, 191, 197, 255, 257, 320, 449, 705, 4160, 8256)


# ------------------------------------------------------------------------------------------------------------------------ masks
def rule_operands(c: Case):
    """(doc_ids int32 [B, S] or None, prefix_len int32 [B] or None): attn_cases.dense_mask's documents and prefixes, the documents
    of batch element b cut once more at S // 5 + 11 b, so that every element has ids and a prefix of its own."""
    _, doc, prefix = A.dense_mask(c.mask, c.B, c.S)
    if doc is not None:
        doc = doc[None].expand(c.B, c.S).clone()
        for b in range(1, c.B):
            doc[b, min(c.S - 1, c.S // 5 + 11 * b):] += 1
    if prefix is not None and c.B > 2:
        prefix[2] = min(c.S, c.S // 4 + 1)
    return doc, prefix


def rule_allow(S: int, doc, prefix, B: int) -> torch.Tensor:
    """bool [B, S, S] of allow(q, k) = (k <= q or k < prefix_len[b]) and doc_ids[b, q] == doc_ids[b, k]."""
    idx = torch.arange(S)
    m = (idx[:, None] >= idx[None, :])[None].expand(B, S, S).clone()
    if prefix is not None:
        m |= idx[None, None, :] < prefix.long()[:, None, None]
    if doc is not None:
        m &= doc[:, :, None] == doc[:, None, :]
    return m


def window_of(c: Case, b: int) -> int:
    return (1500 if c.long else 70) + 9 * b


def pad_of(b: int) -> int:
    return 5 + 9 * b


@functools.lru_cache(maxsize=4)
def allow_of(cid: str) -> torch.Tensor:
    """bool [B, S, S]: the pairs the case's mask allows (the dense form `ss` repeats batch element 0)."""
    c = CASES[cid]
    S, B = c.S, c.B
    idx = torch.arange(S)
    causal = idx[:, None] >= idx[None, :]
    if c.mode == "causal" or c.mask == "eqcausal":
        return causal[None].expand(B, S, S).clone()
    if c.mode == "rule":
        doc, prefix = rule_operands(c)
        return rule_allow(S, doc, prefix, B)
    m = torch.zeros(B, S, S, dtype=torch.bool)
    for b in range(B):
        bb = 0 if c.form == "ss" else b
        if c.mask == "window":
            m[b] = causal & (idx[None, :] > idx[:, None] - window_of(c, bb))
        elif c.mask == "blocks":  # bidirectional: the own 48-position block and every block whose number differs by a multiple of 3
            blk = (idx + 5 * bb) // (1000 if c.long else 48)
            m[b] = (blk[:, None] - blk[None, :]) % 3 == 0
        elif c.mask == "deadblock":  # no row attends to keys 128 .. 255
            m[b] = causal & ~((idx >= 128) & (idx < 256))[None, :]
            m[b, 128:256, 0:(3 + bb)] = True
        elif c.mask == "leftpad":  # keys below pad_of(b) are padding; the rows there have no key at all
            m[b] = causal & (idx >= pad_of(bb))[None, :]
    return m


def keyless_rows(cid: str) -> torch.Tensor:
    """bool [B, S]: the rows without any allowed key - the only rows whose dq is not compared."""
    return ~allow_of(cid).any(-1)


def mask_tensor(c: Case, allow: torch.Tensor, device=None) -> torch.Tensor:
    """The bool mask in the form the case hands to attn_mask_bwd: [S, S], [B, 1, S, S], or the latter as a view of rows S + 12 wide."""
    a = allow if device is None else allow.to(device)
    if c.form == "ss":
        return a[0].contiguous()
    if c.form == "b1ss":
        return a[:, None].contiguous()
    wide = torch.ones(c.B, 1, c.S, c.S + 12, dtype=torch.bool, device=a.device)  # (the bytes beyond a row say "attend")
    wide[..., :c.S] = a[:, None]
    return wide[..., :c.S]


tile_classes = I.tile_classes  # uint8 [B, ceil(S / 128), ceil(S / 64)]: llx_attn_tile_flags and llx_attn_mask_tile_flags agree on it


@functools.lru_cache(maxsize=None)
def flags_of(cid: str) -> torch.Tensor:
    return tile_classes(allow_of(cid))


def families_of(c: Case) -> tuple:
    """The backward families a case runs: all five; at the two long shapes one plane of each census orientation and the selection
    (the low planes tell nothing new about a flag chunk 4096 keys or 8192 rows away, and each family costs a second there)."""
    return ("cenA1", "cenB0", "sel") if c.long else BWD_FAMILIES


# ------------------------------------------------------------------------------------------------------------------------ dispatch
def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def causal_dq_class(qb: int, t: int) -> int:
    return 2 if t * BKV + BKV - 1 <= qb * BQ else 1


def causal_dq_kt_end(S: int, qb: int) -> int:
    return min(cdiv(S, BKV), (qb * BQ + BQ + BKV - 1) // BKV)


def causal_dkv_class(qt: int, kt: int) -> int:
    q_lo, q_hi, k_lo, k_hi = qt * DKV_QT, qt * DKV_QT + DKV_QT - 1, kt * BKV, kt * BKV + BKV - 1
    return 0 if k_lo > q_hi else (2 if k_hi <= q_lo else 1)


def bwd_route(c: Case, ds: bool) -> str:
    """The route llx_attn_bwd takes: b without a dS buffer, with a dense mask, under dropout, and for flagged masks beyond 128 key tiles."""
    if not ds or c.mode == "mask" or (c.mode == "rule" and cdiv(c.S, BKV) > 128):
        return "b"
    return "a"


def classes_of(c: Case) -> set:
    """Every class the restated launchers distinguish that this case makes live."""
    S, nkt, nqb, nqt, nkb = c.S, cdiv(c.S, BKV), cdiv(c.S, BQ), cdiv(c.S, DKV_QT), cdiv(c.S, DKV_KEYS)
    flagged = c.mode != "causal"
    out = {f"mode.{c.mode}", f"G.{c.G}", f"KVH.{c.KVH}", f"B.{c.B}", f"S.{S}"}
    out.add("dq.rope" if c.rope else "dq.norope")
    out.add("dq.store.narrow" if c.narrow else "dq.store.wide")
    out.add(f"{c.mode}.dq.rows." + ("ragged" if S % BQ else "full"))
    out.add(f"{c.mode}.keys." + ("ragged" if S % BKV else "full"))
    out.add(f"{c.mode}.dkv.rows." + ("ragged" if S % DKV_QT else "full"))
    if nqb > 1:
        out.add(f"{c.mode}.blocks.many")
    if nkt % 2:
        out.add(f"{c.mode}.dkv.kt_past_end")
    if not flagged and nkb > 1:
        out.add("causal.dkv.qt_first")
    if c.mode != "mask":
        out.add(f"{c.mode}.fwd.rows." + ("ragged" if S % FWD_ROWS else "full"))
        if cdiv(S, FWD_ROWS) > 1:
            out.add(f"{c.mode}.fwd.blocks.many")
        if c.narrow:
            out.add("fwd.store.narrow")
    if flagged:
        fl = flags_of(c.id)
        out |= {f"{c.mode}.tile.{v}" for v in fl.unique().tolist()}
        # a run of class-0 tiles between two live ones: next_tile / next_qt skip it
        for row in fl.reshape(-1, nkt).tolist():
            live = [i for i, v in enumerate(row) if v]
            if live and any(v == 0 for v in row[live[0]:live[-1]]):
                out.add(f"{c.mode}.dq.skip_run")
        if nkt > 64:
            out.add(f"{c.mode}.dq.flag_reload")
        if nqb > 64:
            out.add(f"{c.mode}.dkv.flag_reload")
        if c.mode == "rule" and c.B > 1:
            doc, prefix = rule_operands(c)
            if prefix is not None and len(set(prefix.tolist())) > 1:
                out.add("rule.prefix.per_batch")
            if doc is not None and not torch.equal(doc[0], doc[1]):
                out.add("rule.doc.per_batch")
    if c.mode == "mask":
        out.add(f"mask.form.{c.form}")
        out.add("mask.m_sb.0" if c.form == "ss" else "mask.m_sb.batch")
        out.add("mask.m_sq.wide" if c.form == "strided" else "mask.m_sq.S")
        if S % 4:
            out.add("mask.S%4" + (".strided" if c.form == "strided" else ""))
        if S == 4:
            out.add("mask.S4")
        if S % BKV:
            out.add("mask.dq.ragged_word")
        if S % 32:
            out.add("mask.dkv.word_clamp")
        if (S - 1) // 32 % 4 != 3:
            out.add("mask.dkv.wave_past_end")
        fl = flags_of(c.id)
        if any(bool(fl[:, qb, t].any()) for qb in range(nqb) for t in range(nkt) if t * BKV > qb * BQ + BQ - 1):
            out.add("mask.above_diagonal")
        if any(not bool(fl[b, :, 2 * kb:2 * kb + 2].any()) for b in range(c.B) for kb in range(nkb)):
            out.add("mask.dkv.dead_block")
        if bool(keyless_rows(c.id).any()):
            out.add("mask.keyless_rows")
    if c.route_a:
        r = bwd_route(c, True)
        out.add(f"a.{c.mode}" if r == "a" else "a.fallback")
        if r == "a":
            out.add("a.Sp." + ("pad" if S % 256 else "full"))
            if cdiv(S, DQ2_ROWS) > 1:
                out.add("a.blocks.many")
            if c.rope:
                out.add("a.rope")
    if c.dropout:
        out.add(f"drop.{c.mode}")
    return out


def required_classes() -> set:
    req = {f"S.{s}" for s in SIZES} | {f"G.{g}" for g in (1, 2, 4, 8)} | {f"KVH.{k}" for k in (1, 2, 3)} | {f"B.{b}" for b in (1, 2, 3)}
    req |= {"dq.rope", "dq.norope", "dq.store.narrow", "dq.store.wide", "fwd.store.narrow", "causal.dkv.qt_first"}
    for m in ("causal", "rule", "mask"):
        req |= {f"mode.{m}", f"{m}.dq.rows.ragged", f"{m}.keys.ragged", f"{m}.keys.full", f"{m}.dkv.rows.ragged",
                f"{m}.dkv.rows.full", f"{m}.blocks.many", f"{m}.dkv.kt_past_end"}
    for m in ("causal", "rule"):
        req |= {f"{m}.fwd.rows.ragged", f"{m}.fwd.blocks.many", f"drop.{m}", f"a.{m}"}
    for m in ("rule", "mask"):
        req |= {f"{m}.tile.0", f"{m}.tile.1", f"{m}.tile.2", f"{m}.dq.skip_run", f"{m}.dq.flag_reload", f"{m}.dkv.flag_reload"}
    req |= {"rule.prefix.per_batch", "rule.doc.per_batch", "a.fallback", "a.Sp.pad", "a.blocks.many", "a.rope"}
    req |= {f"mask.form.{f}" for f in ("ss", "b1ss", "strided")}
    req |= {"mask.m_sb.0", "mask.m_sb.batch", "mask.m_sq.wide", "mask.m_sq.S", "mask.S%4", "mask.S%4.strided", "mask.S4", "mask.dq.ragged_word",
            "mask.dkv.word_clamp", "mask.dkv.wave_past_end", "mask.above_diagonal", "mask.dkv.dead_block", "mask.keyless_rows"}
    return req


# ------------------------------------------------------------------------------------------------------------------------ operands
def _h(seed: int, *xs) -> torch.Tensor:
    """A hash of integer tensors (broadcast together) into 0 .. 2^31 - 1."""
    a = torch.full((), (seed * 0x9E3779B1) % (1 << 31), dtype=torch.int64)
    for i, x in enumerate(xs):
        a = ((a ^ (x.long() + 0x632BE5AB * (i + 1))) * 0x2545F491) % (1 << 31)
        a = a ^ (a >> 13)
    return a


def _seed(cid: str, what: str) -> int:
    return zlib.crc32(f"{cid}/{what}".encode())


def _grid(*ns):
    return torch.meshgrid(*[torch.arange(n) for n in ns], indexing="ij")


def q_salt(c: Case, b, h):
    return ((b * c.H + h) * 7 + 1) % 64


def k_salt(c: Case, b, kvh):
    return ((b * c.KVH + kvh) * 11 + 3) % 64


def do_dim(c: Case, b, q, h):
    return (q + 37 * h + 11 * b) % HD


def rope_table(c: Case) -> torch.Tensor:
    """fp32 [S, 64, 2]: (cos, sin) a quarter turn times a hash of (position, pair)."""
    s, p = _grid(c.S, 64)
    r = _h(_seed(c.id, "rope"), s, p) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[r]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[r]
    return torch.stack([cos, sin], -1).contiguous()


def rope_transpose(x: torch.Tensor, table: torch.Tensor, shift: int = 0) -> torch.Tensor:
    """The dq / dk epilogue on bf16 x [B, S, heads, 128]: the transpose of apply_rope with the table row of position (s + shift) % S."""
    S = x.shape[1]
    t = table[:S].roll(-shift, 0) if shift else table[:S]
    xf = x.float().view(*x.shape[:3], 64, 2)
    cs, sn = t[None, :, None, :, 0], t[None, :, None, :, 1]
    out = torch.stack([xf[..., 0] * cs + xf[..., 1] * sn, xf[..., 1] * cs - xf[..., 0] * sn], -1)
    return out.view(x.shape).to(BF16)


def pick_targets(c: Case, allow: torch.Tensor, seed: int) -> torch.Tensor:
    """int64 [B, H, S]: for every row a key its mask allows - the first, the last or a hashed one - and -1 for a row without keys."""
    B, H, S = c.B, c.H, c.S
    n = allow.sum(-1)  # [B, S]
    tgt = torch.empty(B, H, S, dtype=torch.int64)
    rank = allow.to(torch.int32).cumsum(-1)
    b, q = _grid(B, S)
    for h in range(H):
        r = _h(seed, b, q, torch.tensor(h))
        kind = r % 4
        want = torch.where(kind == 0, torch.ones_like(n), torch.where(kind == 1, n, 1 + (r >> 3) % n.clamp_min(1)))
        tgt[:, h] = ((rank == want[..., None].to(torch.int32)) & allow).to(torch.uint8).argmax(-1)
        tgt[:, h][n == 0] = -1
    return tgt


@functools.lru_cache(maxsize=6)
def build(cid: str, fam: str) -> dict:
    """Backward operands in the kernels' layout - q, o, do [B, S, H, 128], k, v [B, S, KVH, 128] (bf16), lse fp32 [B, H, S] (log2 units) -
    with allow [B, S, S] and keyless [B, S]; asserts the operand ranges the family's exactness rests on."""
    c = CASES[cid]
    B, S, H, KVH, G = c.B, c.S, c.H, c.KVH, c.G
    assert fam in BWD_FAMILIES and S <= 8320
    allow = allow_of(cid)
    keyless = ~allow.any(-1)
    assert c.mask == "leftpad" or not bool(keyless.any())
    d = {"case": c, "fam": fam, "allow": allow, "keyless": keyless}
    b4, s4, h4 = _grid(B, S, H)
    b3, s3, k3 = _grid(B, S, KVH)
    sd = functools.partial(_seed, cid)
    v = ((_h(sd("v"), *_grid(B, S, KVH, HD)) % 7) - 3).float()
    if fam in CEN:
        qoff, koff = (0, 64) if fam[3] == "A" else (64, 0)
        code = (lambda i: i % 64) if fam[4] == "0" else (lambda i: (i // 64) % 64)
        q = torch.zeros(B, S, H, HD)
        q[b4, s4, h4, qoff + (code(s4) + q_salt(c, b4, h4)) % 64] = 1.0
        k = torch.zeros(B, S, KVH, HD)
        k[b3, s3, k3, koff + (code(s3) + k_salt(c, b3, k3)) % 64] = 1.0
        L = (_h(sd("lse"), b4, s4, h4) % 4).float()
        do = torch.zeros(B, S, H, HD)
        do[b4, s4, h4, do_dim(c, b4, s4, h4)] = 1.0
        o = ((_h(sd("o"), *_grid(B, S, H, HD)) % 3) - 1).float()
        lse = L.permute(0, 2, 1).contiguous()
        assert float((q * k.repeat_interleave(G, 2)).abs().sum()) == 0.0  # disjoint halves: every score is 0
        d["dsmax"] = 7.0 if c.dropout else 4.0
    else:
        tgt = pick_targets(c, allow, sd("tgt"))
        salts = torch.tensor([[I.salt(c, b, h // G) for h in range(H)] for b in range(B)])
        ksalt = torch.tensor([[I.salt(c, b, kv) for kv in range(KVH)] for b in range(B)])
        assert S <= 1 << I.CODE_BITS and len(set(ksalt.flatten().tolist())) == B * KVH
        k = O.randn(f"ta_k_{cid}", (B, S, KVH, HD), 1.0).to(BF16).float()
        k[..., :I.CODE_BITS] = I._code(torch.arange(S)[None, :, None] ^ ksalt[:, None, :])
        mag = torch.where(_h(sd("mag"), b4, s4, h4) % 2 == 0, 32.0, 24.0)
        q = torch.zeros(B, S, H, HD)
        tq = tgt.permute(0, 2, 1)  # [B, S, H]
        q[..., :I.CODE_BITS] = I._code(tq.clamp_min(0) ^ salts[:, None, :]) * (mag / 32.0)[..., None]
        q[tq < 0] = 0.0
        do = torch.zeros(B, S, H, HD)
        for j in range(8):
            dim = _h(sd("dodim"), b4, s4, h4, torch.tensor(j)) % HD
            do[b4, s4, h4, dim] = ((_h(sd("doval"), b4, s4, h4, torch.tensor(j)) % 5) - 2).float()
        o = torch.zeros(B, S, H, HD)
        score = (I.CODE_BITS * 32.0 * mag).double() * SCALE_LOG2_32.double()
        lse = score.float().permute(0, 2, 1).contiguous()
        assert bool((allow[:, None].expand(B, H, S, S).gather(3, tgt.clamp_min(0)[..., None])[..., 0] | (tgt < 0)).all())
        d.update(tgt=tgt, mag=mag)
        d["dsmax"] = 8 * 2 * 3.0 * (2 if c.dropout else 1)  # integers below 256: bf16 values
    lse = lse.masked_fill(keyless[:, None, :].expand(B, H, S), float("-inf"))
    for t in (q, k, v, o, do):  # every MFMA operand is a bf16 value
        assert torch.equal(t.to(BF16).float(), t)
    d.update(q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), o=o.to(BF16), do=do.to(BF16), lse=lse)
    if c.rope:
        d["rope"] = rope_table(c)
    return d


def keep_host(c: Case, seed: int = 0) -> torch.Tensor:
    """A stand-in for kernels.attn_dropout_keep on the CPU (uint8 [B, H, S, S]): the CPU proofs need some keep pattern, the GPU test
    takes the kernels' own."""
    b, h, q, k = _grid(c.B, c.H, c.S, c.S)
    return (_h(_seed(c.id, "keep") + seed, b, h, q, k) % 2).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------------ the walks
WALK_FAULTS = ("chunk_skip", "class1_as_2", "ragged_keys", "ragged_rows", "mask_word_shift", "other_prefix", "ds_pad_rows")
EVAL_FAULTS = ("partial_missing", "head_mod", "delta_neighbour", "lse_neighbour", "keep_transposed", "drop_on_ds", "rope_position")
FAULTS = WALK_FAULTS + EVAL_FAULTS


def _pred(c: Case, allow: torch.Tensor, fault: str) -> torch.Tensor:
    """The predicate a class-1 tile evaluates: the mask, or what a fault makes of it."""
    if fault == "other_prefix" and c.mode == "rule":
        doc, prefix = rule_operands(c)
        return rule_allow(c.S, doc, prefix.roll(1), c.B)
    if fault == "mask_word_shift" and c.mode == "mask" and c.S % BKV:
        p = allow.clone()
        t0 = c.S // BKV * BKV
        p[:, :, t0 + 1:] = allow[:, :, t0:-1]  # the ragged tile's bits one key late
        p[:, :, t0] = False
        return p
    return allow


@functools.lru_cache(maxsize=8)
def walk_dq(cid: str, fault: str = "") -> torch.Tensor:
    """uint8 [B, S, S]: how often the tile walk of attn_bwd_dq_kernel (and of the forward, whose tiles and classes are the same) lets
    row q count key k.  Without a fault this is the mask."""
    c = CASES[cid]
    S, nqb, nkt = c.S, cdiv(c.S, BQ), cdiv(c.S, BKV)
    allow = allow_of(cid)
    pred = _pred(c, allow, fault)
    flags = flags_of(cid).tolist() if c.mode != "causal" else None
    W = torch.zeros(c.B, S, S, dtype=torch.uint8)
    for b in range(c.B):
        for qb in range(nqb):
            r = slice(qb * BQ, min(S, qb * BQ + BQ))
            kt_end = nkt if flags else causal_dq_kt_end(S, qb)
            cls = [flags[b][qb][t] if flags else causal_dq_class(qb, t) for t in range(kt_end)]
            if fault == "chunk_skip" and flags:
                cls = [0 if t and t % 64 == 0 else v for t, v in enumerate(cls)]
            ones = [t for t, v in enumerate(cls) if v == 1]
            for t, v in enumerate(cls):
                if v == 0:
                    continue
                ks = slice(t * BKV, min(S, t * BKV + BKV))
                if v == 2 or (fault == "class1_as_2" and t == ones[-1]):
                    W[b, r, ks] += 1
                else:
                    W[b, r, ks] += pred[b, r, ks]
                if fault == "ragged_keys" and t * BKV + BKV > S:  # the clamped keys counted where key S - 1 is
                    W[b, r, S - 1] += (t * BKV + BKV - S) * pred[b, r, S - 1]
    return W


@functools.lru_cache(maxsize=8)
def walk_dkv(cid: str, fault: str = "") -> torch.Tensor:
    """uint8 [B, S, S] (row q, key k): how often the walk of attn_bwd_dkv3_kernel lets key k count row q.  Without a fault: the mask."""
    c = CASES[cid]
    S, nkt, nqt, nkb = c.S, cdiv(c.S, BKV), cdiv(c.S, DKV_QT), cdiv(c.S, DKV_KEYS)
    allow = allow_of(cid)
    pred = _pred(c, allow, fault)
    flags = flags_of(cid).tolist() if c.mode != "causal" else None
    W = torch.zeros(c.B, S, S, dtype=torch.uint8)
    for b in range(c.B):
        for kblk in range(nkb):
            for kt in (2 * kblk, 2 * kblk + 1):
                if kt >= nkt:
                    continue
                ks = slice(kt * BKV, min(S, kt * BKV + BKV))
                for qt in range(0 if flags else (kblk * DKV_KEYS) // DKV_QT, nqt):
                    v = flags[b][qt >> 1][kt] if flags else causal_dkv_class(qt, kt)
                    if fault == "chunk_skip" and flags and (qt >> 1) and (qt >> 1) % 64 == 0:
                        v = 0
                    if v == 0:
                        continue
                    ragged = qt * DKV_QT + DKV_QT > S
                    r = slice(qt * DKV_QT, min(S, qt * DKV_QT + DKV_QT))
                    if (v == 2 and not ragged) or (fault == "class1_as_2" and v == 1 and kt == max(t for t in range(nkt) if (flags[b][qt >> 1][t] if flags else causal_dkv_class(qt, t)) == 1)):
                        W[b, r, ks] += 1
                    else:
                        W[b, r, ks] += pred[b, r, ks]
                    if fault in ("ragged_rows", "ds_pad_rows") and ragged:  # the clamped rows counted where row S - 1 is
                        W[b, S - 1, ks] += (qt * DKV_QT + DKV_QT - S) * pred[b, S - 1, ks]
    return W


def fault_applies(c: Case, fault: str, route: str = "b") -> bool:
    """Whether the case (on the given route) is aimed at the fault's class.  The long shapes exist for the flag reloads: they are
    aimed at the chunk-boundary fault alone (the other classes are live at the short shapes, where a check costs a hundredth)."""
    S = c.S
    if c.long and fault != "chunk_skip":
        return False
    flagged = c.mode != "causal"
    if fault == "chunk_skip":
        if not flagged:
            return False
        fl = flags_of(c.id)
        # (route (a) keeps the dQ schedule in two 64-bit masks: only the dK/dV walk reloads there)
        return (route == "b" and cdiv(S, BKV) > 64 and bool(fl[:, :, 64::64].any())) or (cdiv(S, BQ) > 64 and bool(fl[:, 64::64].any()))
    return {"class1_as_2": S > 1, "ragged_keys": S % BKV != 0 and route == "b", "ragged_rows": S % DKV_QT != 0 and S > 1,
            "mask_word_shift": c.mode == "mask" and S % BKV > 1, "other_prefix": c.mode == "rule" and "prefix" in c.mask and c.B > 1,
            "ds_pad_rows": route == "a" and S % DKV_QT != 0 and S > 1, "partial_missing": c.G > 1, "head_mod": c.G > 1 and c.KVH > 1,
            "delta_neighbour": S > 1, "lse_neighbour": S > 1, "keep_transposed": c.dropout and route == "b" and S > 1,
            "drop_on_ds": c.dropout and route == "b", "rope_position": c.rope and S > 1}[fault]


# ------------------------------------------------------------------------------------------------------------------------ references
def _rb(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF16).to(x.dtype)


def evaluate(d: dict, Wq=None, Wkv=None, *, fault: str = "", keep=None, dtype=torch.float32, operand_rounding: bool = True, check=None):
    """The backward as the kernels document it, on weights: row q counts key k Wq[b, q, k] times in dQ and Wkv[b, q, k] times in dK / dV
    (None: the mask).  P = exp2(s . scale_log2 - lse) with -inf lse read as 0, delta = rowsum(dO . O), dP doubled where kept under dropout
    (keep uint8 [B, H, S, S]), dS = P (dP - delta); bf16 P feeds dV and bf16 dS feeds dQ and dK (operand_rounding), fp32 partials per
    head, dq / dk = bf16(fl32(sum) . fl32(scale)), dv = bf16(sum), then the rope epilogue.  Returns bf16 (dq, dk, dv) in the operands'
    layouts.  `fault`: one of EVAL_FAULTS.  `check`: a dict that receives the largest |dS|, the largest partial sum, and whether
    rounding P and dS to bf16 changed any value."""
    c = d["case"]
    B, S, H, KVH, G = c.B, c.S, c.H, c.KVH, c.G
    allow = d["allow"]
    q, k, v, o, do = (d[n].to(dtype) for n in ("q", "k", "v", "o", "do"))
    lse = torch.where(torch.isinf(d["lse"]), torch.zeros_like(d["lse"]), d["lse"]).to(dtype)
    delta = (do * o).sum(-1).permute(0, 2, 1)  # [B, H, S]
    if fault == "delta_neighbour":
        delta = delta.roll(-1, 2)
    if fault == "lse_neighbour":
        lse = lse.roll(-1, 2)
    c2 = SCALE_LOG2_32.to(dtype)
    dq = torch.zeros(B, S, H, HD, dtype=dtype)
    pk = torch.zeros(B, H, S, HD, dtype=dtype)
    pv = torch.zeros(B, H, S, HD, dtype=dtype)
    rnd = (lambda x: _rb(x)) if operand_rounding else (lambda x: x)
    stats = {"ds": 0.0, "sum": 0.0, "inexact": False}
    for b in range(B):
        for h in range(H):
            kv = h % KVH if fault == "head_mod" else h // G
            kk, vv = k[b, :, kv], v[b, :, kv]
            for r0 in range(0, S, 1024):
                r = slice(r0, min(S, r0 + 1024))
                wq = (allow if Wq is None else Wq)[b, r].to(dtype)
                wk = (allow if Wkv is None else Wkv)[b, r].to(dtype)
                live = (wq > 0) | (wk > 0)
                arg = (q[b, r, h] @ kk.T) * c2 - lse[b, h, r, None]
                P = torch.where(live, torch.exp2(arg.clamp_max(100.0)), torch.zeros_like(arg))
                dP = do[b, r, h] @ vv.T
                Pd = P
                if keep is not None:
                    kp = (keep[b, h].T[r] if fault == "keep_transposed" else keep[b, h, r]).to(dtype) * 2.0
                    dP = dP * kp
                    Pd = P * kp
                dS = (Pd if fault == "drop_on_ds" else P) * (dP - delta[b, h, r, None])
                Pb, dSb = rnd(Pd), rnd(dS)
                if check is not None:
                    stats["ds"] = max(stats["ds"], float((dS * live).abs().max()))
                    stats["inexact"] |= not (torch.equal(Pb, Pd) and torch.equal(dSb, dS))
                dq[b, r, h] = (wq * dSb) @ kk
                pv[b, h] += (wk * Pb).T @ do[b, r, h]
                pk[b, h] += (wk * dSb).T @ q[b, r, h]
    if check is not None:
        stats["sum"] = max(float(dq.abs().max()), float(pk.abs().max()), float(pv.abs().max()))
        check.update(stats)
    pk, pv = pk.view(B, KVH, G, S, HD), pv.view(B, KVH, G, S, HD)
    if fault == "head_mod":  # the partial of head h lands with kv head h % KVH
        pk = pk.reshape(B, H, S, HD)[:, [[h for h in range(H) if h % KVH == kv] for kv in range(KVH)]]
        pv = pv.reshape(B, H, S, HD)[:, [[h for h in range(H) if h % KVH == kv] for kv in range(KVH)]]
    if fault == "partial_missing":
        pk, pv = pk[:, :, :-1], pv[:, :, :-1]
    dk = (pk.sum(2).float() * SCALE32).permute(0, 2, 1, 3).to(BF16)  # (the sums are fp32 values; the product is an fp32 product)
    dv = pv.sum(2).permute(0, 2, 1, 3).to(BF16)
    dq = (dq.float() * SCALE32).to(BF16)
    if "rope" in d:
        shift = 1 if fault == "rope_position" else 0
        dq, dk = rope_transpose(dq, d["rope"], shift), rope_transpose(dk, d["rope"], shift)
    return dq.contiguous(), dk.contiguous(), dv.contiguous()


def expected(cid: str, fam: str, keep=None) -> tuple:
    """(dq, dk, dv) bf16 for the case's operands, from the mask itself; asserts the exactness bounds: every dS and P is a bf16 value,
    |dS| within the family's bound and every sum below 2^21 (a multiple of 2^-3 below 2^24 2^-3 is exact in fp32 in any order)."""
    d = build(cid, fam)
    st = {}
    out = evaluate(d, keep=keep, check=st)
    assert not st["inexact"] and st["ds"] <= d["dsmax"] and st["sum"] < 2.0 ** 21, (cid, fam, st)
    return out


def ref64(d: dict, keep=None) -> tuple:
    """The plain float64 backward with the given o and lse, whole [B, H, S, S] tensors (a second statement of
    the formula: attn_cases.bwd64 with P = exp2(s . scale_log2 - lse) instead of its own softmax), outputs rounded as documented."""
    c = d["case"]
    B, S, H, KVH, G = c.B, c.S, c.H, c.KVH, c.G
    q, o, do = (d[n].double().transpose(1, 2) for n in ("q", "o", "do"))
    k, v = (d[n].double().transpose(1, 2).repeat_interleave(G, 1) for n in ("k", "v"))
    lse = torch.where(torch.isinf(d["lse"]), torch.zeros_like(d["lse"]), d["lse"]).double()
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * SCALE_LOG2_32.double() - lse[..., None]
    P = torch.exp2(s.clamp_max(100.0)).masked_fill(~d["allow"][:, None], 0.0)
    dP = torch.einsum("bhqd,bhkd->bhqk", do, v)
    Pd = P
    if keep is not None:
        dP, Pd = dP * keep.double() * 2.0, P * keep.double() * 2.0
    dS = _rb(P * (dP - (do * o).sum(-1, keepdim=True)))  # the two documented operand roundings: bf16 dS into dQ / dK, bf16 P into dV
    Pd = _rb(Pd)
    fold = lambda x: x.view(B, KVH, G, S, HD).sum(2).transpose(1, 2)
    dq = (torch.einsum("bhqk,bhkd->bhqd", dS, k).float() * SCALE32).transpose(1, 2).to(BF16)
    dk = (fold(torch.einsum("bhqk,bhqd->bhkd", dS, q)).float() * SCALE32).to(BF16)
    dv = fold(torch.einsum("bhqk,bhqd->bhkd", Pd, do)).to(BF16)
    if "rope" in d:
        dq, dk = rope_transpose(dq, d["rope"]), rope_transpose(dk, d["rope"])
    return dq.contiguous(), dk.contiguous(), dv.contiguous()


def same(got: tuple, want: tuple, keyless: torch.Tensor) -> list:
    """The names of the gradients that differ (torch.equal; the dq rows of keyless rows left out)."""
    bad = []
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        if name == "dq" and bool(keyless.any()):
            g, w = g.masked_fill(keyless[:, :, None, None], 0), w.masked_fill(keyless[:, :, None, None], 0)
        if not torch.equal(g, w):
            bad.append(name)
    return bad


def explain(got: tuple, want: tuple, keyless: torch.Tensor, limit: int = 6) -> str:
    """The first rows that miss, by name: gradient, (b, position, head) and the first differing dims."""
    lines = []
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        ne = (g.float() != w.float()) | (torch.isnan(g.float()) != torch.isnan(w.float()))
        if name == "dq":
            ne &= ~keyless[:, :, None, None]
        rows = ne.any(-1).nonzero()
        for b, s, h in rows[:limit].tolist():
            dims = ne[b, s, h].nonzero().flatten()[:4].tolist()
            lines.append(f"{name}[b {b}, pos {s}, head {h}] ({len(rows)} rows differ) dims {dims}: got {g[b, s, h, dims].tolist()} want {w[b, s, h, dims].tolist()}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=4)
def build_fwd(cid: str, fam: str) -> dict:
    """The sel / cen0 / cen1 operands of tests/infer_attn_cases.py for a causal or rule case, in that module's layout (q [B, H, S, 128],
    k / v [B, KVH, S, 128]) with its expectation keys (want + tgt, or count + count_d), so that its reference and decoders apply."""
    c = CASES[cid]
    B, S, H, KVH, G = c.B, c.S, c.H, c.KVH, c.G
    assert c.mode != "mask" and fam in FWD_FAMILIES and S <= 1 << I.CODE_BITS
    allow = allow_of(cid)
    m4 = allow[:, None].expand(B, H, S, S)
    d = {"case": c, "fam": fam, "mask4": m4, "allow": allow}
    keys = torch.arange(S)
    if fam == "sel":
        tgt = pick_targets(c, allow, _seed(cid, "ftgt"))
        k = O.randn(f"ta_fk_{cid}", (B, KVH, S, HD), 1.0)
        for b in range(B):
            for kv in range(KVH):
                k[b, kv, :, :I.CODE_BITS] = I._code(keys ^ I.salt(c, b, kv))
        salts = torch.tensor([[I.salt(c, b, h // G) for h in range(H)] for b in range(B)])
        q = torch.zeros(B, H, S, HD)
        q[..., :I.CODE_BITS] = I._code(tgt ^ salts[:, :, None])
        v = O.randn(f"ta_fv_{cid}", (B, KVH, S, HD), 1.0).to(BF16)
        want = v.repeat_interleave(G, 1).gather(2, tgt[..., None].expand(B, H, S, HD)).clone()
        assert int(tgt.min()) >= 0 and bool(m4.gather(3, tgt[..., None]).all())
        d.update(q=q.to(BF16), k=k.to(BF16), v=v, tgt=tgt, want=want)
    else:
        k = O.randn(f"ta_fkc_{cid}", (1, 1, S, HD), 50.0).expand(B, KVH, S, HD).clone()
        k.view(-1)[::37] = 1e4
        idx = keys % HD if fam == "cen0" else (keys // HD) % HD
        v1 = torch.zeros(S, HD)
        v1[keys, idx] = 1.0
        count = m4.sum(-1)
        count_d = (allow.float() @ v1).round().long()[:, None].expand(B, H, S, HD)
        assert int(count_d.max()) <= 128 and torch.equal(count_d.sum(-1), count)
        d.update(q=torch.zeros(B, H, S, HD, dtype=BF16), k=k.to(BF16), v=v1.to(BF16).expand(B, KVH, S, HD).contiguous(), count=count, count_d=count_d)
    return d


def fwd_dropout_ok(o: torch.Tensor, d: dict, keep: torch.Tensor) -> bool:
    """Census under dropout at p = 1/2: o [B, H, S, 128] is twice the kept count per dim over the row's count.  Decoded as
    round(o count / 2) == kept_d (halving is exact): bf16 leaves a relative 2^-8 at most, which cannot move an integer up to 127."""
    v1 = d["v"][0, 0].float()
    kept = torch.einsum("bhqk,kd->bhqd", (keep.bool() & d["mask4"]).float(), v1).round().long()
    assert int(kept.max()) <= 127
    return bool(torch.equal(torch.round(o.double() * d["count"][..., None] / 2).long(), kept))
