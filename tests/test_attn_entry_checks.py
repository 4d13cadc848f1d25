"""CPU: the argument checks of the four training-attention entry points (llx_attn_fwd, llx_attn_mask_fwd, llx_attn_bwd,
llx_attn_mask_bwd).  Validation runs before any launch, so dummy pointers and a null stream are enough.  Each case changes ONE
argument of an otherwise valid call and must be refused (-1) with the entry's own name and the condition's keyword in the message.
The entries' checks differ on purpose (o / dq may be 8-byte aligned where the inputs need 16, the mask entries bound Skv, B and the
K/V position strides, ...): the tables below are those differences.  A value one entry accepts where its neighbours refuse cannot be
shown by a passing call (that would launch); it is probed together with the condition the entry checks LAST (S = 2^24; in the mask
entries the overlapping mask rows): the message then names that condition, not the probed argument."""
import ctypes

import pytest

P = ctypes.c_void_p(256)  # aligned for every operand (the dS buffer wants 256)
BIG = 1 << 24
Q_SS, Q_SB, K_SS, K_SB = 4 * 128, 8 * 4 * 128, 128, 8 * 128  # B = 1, S = 8, H = 4, KVH = 1

FWD = dict(q=P, q_sb=Q_SB, q_ss=Q_SS, k=P, k_sb=K_SB, k_ss=K_SS, v=P, v_sb=K_SB, v_ss=K_SS, o=P, o_sb=Q_SB, o_ss=Q_SS, lse=P, doc_ids=None,
           prefix_len=None, flags=None, B=1, S=8, H=4, KVH=1, head_dim=128, scale=0.1, stream=None)
MASK_FWD = dict(q=P, q_sb=Q_SB, q_ss=Q_SS, k=P, k_sb=K_SB, k_sh=128, k_ss=K_SS, v=P, v_sb=K_SB, v_sh=128, v_ss=K_SS, o=P, o_sb=Q_SB, o_ss=Q_SS,
                lse=P, mask=P, m_sb=0, m_sq=16, flags=P, B=1, Sq=8, Skv=16, H=4, KVH=1, head_dim=128, scale=0.1, stream=None)
_BWD_HEAD = dict(q=P, q_sb=Q_SB, q_ss=Q_SS, k=P, k_sb=K_SB, k_ss=K_SS, v=P, v_sb=K_SB, v_ss=K_SS, o=P, o_sb=Q_SB, o_ss=Q_SS, d_o=P, do_sb=Q_SB,
                 do_ss=Q_SS, lse=P, delta=P, dq=P, dq_sb=Q_SB, dq_ss=Q_SS, dk=P, dk_sb=K_SB, dk_ss=K_SS, dv=P, dv_sb=K_SB, dv_ss=K_SS)
_BWD_TAIL = dict(B=1, S=8, H=4, KVH=1, head_dim=128, scale=0.1, stream=None)
BWD = dict(**_BWD_HEAD, doc_ids=None, prefix_len=None, flags=None, rope=None, ds=None, **_BWD_TAIL)
MASK_BWD = dict(**_BWD_HEAD, mask=P, m_sb=0, m_sq=8, flags=P, rope=None, **_BWD_TAIL)
BASE = {"llx_attn_fwd": FWD, "llx_attn_mask_fwd": MASK_FWD, "llx_attn_bwd": BWD, "llx_attn_mask_bwd": MASK_BWD}

p8, p4 = ctypes.c_void_p(8), ctypes.c_void_p(4)
_FWD_COMMON = [
    (dict(q=None), b"null pointer"), (dict(o=None), b"null pointer"),
    (dict(head_dim=64), b"head_dim"), (dict(KVH=3), b"bad B/"), (dict(B=0), b"bad B/"),
    (dict(q_ss=Q_SS + 4), b"strides"), (dict(k_sb=K_SB + 4), b"strides"), (dict(v_ss=K_SS + 4), b"strides"),  # inputs: % 8
    (dict(o_ss=Q_SS + 2), b"strides"), (dict(o_sb=Q_SB + 2), b"strides"),                                      # o: % 4
    (dict(q=p8), b"unaligned"), (dict(k=p8), b"unaligned"), (dict(v=p8), b"unaligned"), (dict(o=p4), b"unaligned"),  # q/k/v % 16, o % 8
]
_BWD_COMMON = [
    (dict(lse=None), b"null pointer"), (dict(delta=None), b"null pointer"), (dict(dv=None), b"null pointer"),
    (dict(head_dim=64), b"head_dim"), (dict(KVH=3), b"bad B/"), (dict(S=0), b"bad B/"),
    (dict(do_ss=Q_SS + 4), b"input strides"), (dict(o_sb=Q_SB + 4), b"input strides"), (dict(k_ss=K_SS + 4), b"input strides"),  # % 8
    (dict(dq_ss=Q_SS + 2), b"output strides"), (dict(dv_sb=K_SB + 2), b"output strides"),                                          # % 4
    (dict(q=p8), b"unaligned input"), (dict(d_o=p8), b"unaligned input"),
    (dict(dq=p4), b"unaligned output"), (dict(dk=p8), b"unaligned output"), (dict(dv=p8), b"unaligned output"),  # dq % 8, dk | dv % 16
    (dict(dk_ss=K_SS + 4), b"unaligned output"), (dict(dv_sb=K_SB + 4), b"unaligned output"),                    # dk / dv strides % 8
    (dict(rope=p8), b"rope"),
    (dict(S=BIG), b"too large"), (dict(B=1 << 14), b"too large"),  # B * H = 2^16
    # accepted where dk / dv are not: dq 8-byte aligned with strides % 4 (S = 2^24 is the last check)
    (dict(dq=p8, S=BIG), b"too large"), (dict(dq_ss=Q_SS + 4, dq_sb=Q_SB + 4, S=BIG), b"too large"),
]
CASES = {
    "llx_attn_fwd": _FWD_COMMON + [
        (dict(S=BIG), b"S too large"),
        (dict(doc_ids=P), b"tile flags required"), (dict(prefix_len=P), b"tile flags required"),
        # accepted: o 8-byte aligned with strides % 4; flags without doc_ids / prefix_len (ignored)
        (dict(o=p8, S=BIG), b"S too large"), (dict(o_ss=Q_SS + 4, o_sb=Q_SB + 4, S=BIG), b"S too large"), (dict(flags=P, S=BIG), b"S too large"),
    ],
    "llx_attn_mask_fwd": _FWD_COMMON + [
        (dict(mask=None), b"null pointer"), (dict(flags=None), b"null pointer"),
        (dict(B=65536), b"bad B/"),
        (dict(Skv=3), b"Skv=3"), (dict(Skv=BIG), b"out of range"), (dict(Sq=BIG), b"out of range"),
        (dict(k_sh=132), b"strides"), (dict(v_sh=132), b"strides"),
        (dict(k_ss=-8), b"position stride"), (dict(v_ss=-8), b"position stride"), (dict(k_ss=BIG), b"position stride"),
        (dict(v_ss=BIG), b"position stride"),
        (dict(m_sq=15), b"mask rows overlap"), (dict(m_sb=-1), b"mask rows overlap"),
        # accepted as in llx_attn_fwd: o 8-byte aligned with strides % 4 (the mask rows are the last check)
        (dict(o=p8, m_sq=15), b"mask rows overlap"), (dict(o_ss=Q_SS + 4, o_sb=Q_SB + 4, m_sq=15), b"mask rows overlap"),
    ],
    "llx_attn_bwd": _BWD_COMMON + [
        (dict(doc_ids=P), b"tile flags required"), (dict(prefix_len=P), b"tile flags required"),
        (dict(ds=ctypes.c_void_p(128)), b"256-byte"),
        (dict(flags=P, S=BIG), b"too large"),  # accepted: flags without doc_ids / prefix_len (ignored)
    ],
    "llx_attn_mask_bwd": _BWD_COMMON + [
        (dict(mask=None), b"null pointer"), (dict(flags=None), b"null pointer"),
        (dict(S=3), b"S=3"),
        (dict(m_sq=7), b"mask rows overlap"), (dict(m_sb=-1), b"mask rows overlap"),
        (dict(dq=p8, m_sq=7), b"mask rows overlap"), (dict(dq_ss=Q_SS + 4, dq_sb=Q_SB + 4, m_sq=7), b"mask rows overlap"),  # accepted, as above
    ],
}


@pytest.mark.parametrize("entry", sorted(CASES))
def test_entry_refuses_each_condition_under_its_own_name(entry):
    from llx import _lib as L

    lib = L.load()
    fn, base = getattr(lib, entry), BASE[entry]
    assert len(base) == len(L.SIGNATURES[entry][1]), "the base call must name every argument, in the ABI's order"
    for change, keyword in CASES[entry]:
        assert set(change) <= set(base), change
        rc = fn(*{**base, **change}.values())
        msg = lib.llx_last_error_string()
        assert rc == -1, (entry, change, rc, msg)
        assert msg.startswith(entry.encode() + b":") and keyword in msg, (entry, change, msg)
