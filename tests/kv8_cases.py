"""The FP8 KV cache format as a numpy oracle, written from the format and not from any conversion routine: OCP E4M3
(e4m3fn) codes - 1 sign bit, 4 exponent bits with bias 7, 3 mantissa bits; normals from 2^-6, subnormals in steps of 2^-9, largest
value 448 = 0x7e, no infinities, 0x7f / 0xff are NaN - without a scale.

    q(x), on a bf16 value x:  clamp to [-448, 448]; round to nearest, ties to even, on the grid; the sign bit is the input's (for zero
                              too); +-inf saturates like any other value; NaN -> a NaN code.
    dq(code):                 exact in bf16 for every code.

A value that starts as fp32 is rounded to bf16 first (the value the bf16 cache would have held) and then to E4M3: the double rounding
is part of the contract.  FAULTS are wrong encoders, each of which must break at least one hand vector (tests/test_kv8_cases.py)."""
import numpy as np
import torch

BF16 = torch.bfloat16
FAULTS = ("truncate", "ties_away", "fnuz_bias", "nan_on_overflow", "flush_subnormals", "from_fp32")


def _bits(x: torch.Tensor) -> np.ndarray:
    """The 16-bit patterns of a bf16 tensor."""
    assert x.dtype is BF16
    return x.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def _values(bits: np.ndarray) -> np.ndarray:
    """bf16 patterns -> their values in float64 (exact)."""
    with np.errstate(invalid="ignore"):  # (signalling NaN patterns)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _encode_values(val: np.ndarray, sign: np.ndarray, fault=None) -> np.ndarray:
    """q() on float64 values `val` with sign bits `sign` (0 / 1; carried separately: -0 has one)."""
    nan = np.isnan(val)
    a = np.abs(np.where(nan, 0.0, val))
    over = a > 448.0
    a = np.minimum(a, 448.0)  # the clamp (+-inf too)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.maximum(e, -6.0)   # below 2^-6: the subnormal grid, steps of 2^-9
    step = np.exp2(e - 3.0)   # 8 steps per binade
    t = a / step              # exact: a power-of-two quotient
    if fault == "truncate":
        n = np.floor(t)
    elif fault == "ties_away":
        n = np.floor(t + 0.5)
    else:
        n = np.rint(t)        # ties to even
    r = n * step              # the rounded magnitude, <= 448
    if fault == "flush_subnormals":
        r = np.where(r < 2.0 ** -6, 0.0, r)
    with np.errstate(divide="ignore"):
        e2 = np.floor(np.log2(np.where(r > 0, r, 1.0)))  # (rounding up may have reached the next binade)
    bias = 8 if fault == "fnuz_bias" else 7
    normal = r >= 2.0 ** -6
    code_n = ((e2 + bias).astype(np.int64) << 3) | np.rint((r / np.exp2(e2) - 1.0) * 8.0).astype(np.int64)
    code_s = np.rint(r * 2.0 ** 9).astype(np.int64)  # subnormal: the count of 2^-9 steps, 0 .. 7
    code = np.where(normal, code_n, code_s)
    if fault == "nan_on_overflow":
        code = np.where(over, 0x7F, code)
    code = np.where(nan, 0x7F, code)
    return (code | (sign.astype(np.int64) << 7)).astype(np.uint8)


def encode(x: torch.Tensor, fault=None) -> torch.Tensor:
    """q(x) for a bf16 tensor -> uint8 codes of the same shape (on the CPU)."""
    bits = _bits(x)
    codes = _encode_values(_values(bits), (bits >> 15) & 1, None if fault == "from_fp32" else fault)
    return torch.from_numpy(codes.reshape(tuple(x.shape)))


def encode_f32(x: torch.Tensor, fault=None) -> torch.Tensor:
    """q() of values that start as fp32: through bf16 (round to nearest even), as the cache's writers do.  fault "from_fp32" skips that step."""
    assert x.dtype is torch.float32
    if fault == "from_fp32":
        v = x.detach().cpu().numpy().astype(np.float64)
        return torch.from_numpy(_encode_values(v, np.signbit(v).astype(np.int64), None).reshape(tuple(x.shape)))
    return encode(x.to(BF16), fault)


def decode(codes: torch.Tensor) -> torch.Tensor:
    """dq(codes) for a uint8 tensor -> bf16 of the same shape (on the CPU); exact."""
    assert codes.dtype is torch.uint8
    c = codes.detach().cpu().contiguous().numpy().astype(np.int64)
    s, e, m = c >> 7, (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2(e - 7.0))
    val = np.where((e == 15) & (m == 7), np.nan, mag) * np.where(s == 1, -1.0, 1.0)
    f32 = val.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), val, equal_nan=True)
    out = torch.from_numpy(f32).to(BF16)
    assert torch.equal(out.float().nan_to_num(nan=7.0), torch.from_numpy(f32).nan_to_num(nan=7.0)), "dq() must be exact in bf16"
    return out.reshape(tuple(codes.shape))


def roundtrip(x: torch.Tensor) -> torch.Tensor:
    """dq(q(x)): what an fp8 cache holds where the bf16 cache holds x (same device and shape as x)."""
    return decode(encode(x)).to(x.device)


def is_nan_code(codes: torch.Tensor) -> torch.Tensor:
    return (codes & 0x7F) == 0x7F


def same_codes(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Equality of code tensors where a NaN code may carry either sign (0x7f and 0xff are both accepted)."""
    got, want = got.cpu(), want.cpu()
    if got.shape != want.shape or got.dtype is not torch.uint8 or want.dtype is not torch.uint8:
        return False
    n = is_nan_code(want)
    return bool(torch.equal(is_nan_code(got), n) and torch.equal(got[~n], want[~n]))


def all_bf16() -> torch.Tensor:
    """All 65 536 bf16 patterns, in pattern order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)


# hand vectors: (name, bf16 input, code); computed by hand from the grid: between 16 and 32 the step is 2, between 256 and 448 it is 32
HAND = [
    ("max", 448.0, 0x7E),
    ("tie_above_max", 464.0, 0x7E),        # clamped, not rounded towards 480
    ("above_max", 480.0, 0x7E),
    ("far_above_max", 9984.0, 0x7E),
    ("tie_17", 17.0, 0x58),                # between 16 (mantissa 000) and 18 (001): to even = 16
    ("exact_18", 18.0, 0x59),
    ("tie_19", 19.0, 0x5A),                # between 18 (001) and 20 (010): to even = 20
    ("min_subnormal", 2.0 ** -9, 0x01),
    ("tie_to_zero", 2.0 ** -10, 0x00),     # between 0 and 2^-9: to even = 0
    ("tie_sub_1p5", 1.5 * 2.0 ** -9, 0x02),
    ("tie_sub_2p5", 2.5 * 2.0 ** -9, 0x02),
    ("small_normal", 0.0175, 0x09),        # bf16(0.0175) = 0.017456..: nearest of 0.015625 (0x08), 0.017578 (0x09), 0.019531 (0x0a)
    ("minus_zero", -0.0, 0x80),
    ("minus_tie_17", -17.0, 0xD8),
    ("plus_inf", float("inf"), 0x7E),
    ("minus_inf", float("-inf"), 0xFE),
    ("one", 1.0, 0x38),
    ("min_normal", 2.0 ** -6, 0x08),
    ("sub_round_to_normal", 7.5 * 2.0 ** -9, 0x08),  # tie between subnormal 7 and the first normal (8 steps): to even = 0x08
]
# fp32 input: 17.01 is above the tie of 16 | 18 and would go to 18, but bf16(17.01) = 17.0 sits on it and goes to 16
HAND_F32 = [("double_rounding_17p01", 17.01, 0x58)]


def hand_codes(fault=None) -> dict:
    """name -> the code the (faulty) encoder gives every hand vector."""
    out = {}
    for name, x, _ in HAND:
        out[name] = int(encode(torch.tensor([x], dtype=torch.float32).to(BF16), fault)[0])
    for name, x, _ in HAND_F32:
        out[name] = int(encode_f32(torch.tensor([x], dtype=torch.float32), fault)[0])
    return out
