"""CPU checks of the FP8 KV cache oracle (tests/kv8_cases.py): the hand vectors, agreement with torch's float8_e4m3fn cast after the
clamp on all 65 536 bf16 patterns and with torch's decode on all 256 codes, and every planted fault breaks at least one hand vector."""
import pytest
import torch

from tests import kv8_cases as C

BF16 = torch.bfloat16


@pytest.mark.parametrize("name", [h[0] for h in C.HAND + C.HAND_F32])
def test_hand_vectors(name):
    want = next(h[2] for h in C.HAND + C.HAND_F32 if h[0] == name)
    assert C.hand_codes()[name] == want, f"{name}: {C.hand_codes()[name]:#04x} != {want:#04x}"


def test_nan_encodes_as_nan_code():
    x = torch.tensor([float("nan"), -float("nan")], dtype=torch.float32).to(BF16)
    c = C.encode(x)
    assert bool(C.is_nan_code(c).all())
    assert bool(C.decode(c).float().isnan().all())


def test_encoder_equals_torch_on_every_bf16_pattern():
    x = C.all_bf16()
    got = C.encode(x)
    want = x.float().clamp(-448.0, 448.0).to(BF16).to(torch.float8_e4m3fn).view(torch.uint8)
    nan = x.float().isnan()
    assert int(nan.sum()) == 2 * 127
    assert torch.equal(got[~nan], want[~nan])  # the sign of -0 and the saturation of +-inf included
    assert bool(C.is_nan_code(got[nan]).all()) and not bool(C.is_nan_code(got[~nan]).any())


def test_decoder_equals_torch_on_every_code():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    got = C.decode(codes)
    want = codes.view(torch.float8_e4m3fn).to(BF16)
    nan = C.is_nan_code(codes)
    assert codes[nan].tolist() == [0x7F, 0xFF]
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))  # bit for bit: the sign of -0 too
    assert bool(got[nan].float().isnan().all()) and bool(want[nan].float().isnan().all())
    # every code is a fixed point of the round trip: q(dq(c)) == c
    assert C.same_codes(C.encode(got), codes)


def test_roundtrip_is_idempotent_and_monotone():
    x = C.all_bf16()
    fin = ~x.float().isnan()
    r = C.roundtrip(x)
    assert torch.equal(C.roundtrip(r)[fin].view(torch.int16), r[fin].view(torch.int16))
    v, order = x.float()[fin].sort(stable=True)
    rv = r.float()[fin][order]
    assert bool((rv[1:] >= rv[:-1]).all()) and float(rv.max()) == 448.0 and float(rv.min()) == -448.0


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_fault_breaks_a_hand_vector(fault):
    want = {h[0]: h[2] for h in C.HAND + C.HAND_F32}
    got = C.hand_codes(fault)
    broken = [n for n in want if got[n] != want[n]]
    assert broken, f"no hand vector notices the fault {fault!r}"
