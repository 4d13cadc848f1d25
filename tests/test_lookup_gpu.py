"""GPU: the lookup-step kernel (csrc/lookup.hip, kernels.lookup_step) against its host reference (sampling.lookup_accept, then
sampling.lookup_draft): every state tensor after one launch, integer for integer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 3, 4, 255, 256, 257, 1025, 2049)  # the 256 threads of the one workgroup, their strides and the reduction all turn over
PAD = -7  # fills seq behind the tokens, and the slack behind cap that the kernel is not told about


def _tokens(length, seed, vocab=5):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, vocab, size=length).tolist()


def _picks(fed, accept, k, vocab_map=None):
    """Picks that confirm exactly `accept` draft tokens of `fed`; the rows behind the first rejection hold tokens of their own."""
    other = (lambda t: (t + 1) % 5) if vocab_map is None else (lambda t: vocab_map[(vocab_map.index(t) + 1) % len(vocab_map)])
    picks = [fed[1 + i] if i < accept else other(fed[min(1 + i, k)]) for i in range(k + 1)]
    if accept == k:
        picks[k] = other(fed[k])
    return picks


def _expect(seq, fed, picks, *, P, n, k, g, eos=None, init=False, counters=(3, 5)):
    from llx.sampling import lookup_accept, lookup_draft

    room = P + n - len(seq)
    emitted, fin = lookup_accept([seq[-1]] + [None] * k, picks[:1], 0, eos, room) if init else lookup_accept(fed, picks, k, eos, room)
    new = seq + emitted
    return dict(seq=new, len=[len(new)], step_tok=[new[-1]] + lookup_draft(new, g, k), step_pos=list(range(len(new) - 1, len(new) + k)),
                finished=[int(fin)], counters=[counters[0] + 1, counters[1] + len(emitted) - 1])


def _state(cuda, seq, fed, *, P, n, k, finished=0, counters=(3, 5)):
    cap = P + n
    buf = torch.full((cap + 4,), PAD, dtype=torch.int64)
    buf[: len(seq)] = torch.tensor(seq, dtype=torch.int64)
    return dict(buf=buf.to(cuda), len=torch.tensor([len(seq)], device=cuda), step_tok=torch.tensor(fed, device=cuda),
                step_pos=torch.arange(len(seq) - 1, len(seq) + k, device=cuda), finished=torch.tensor([finished], dtype=torch.int32, device=cuda),
                counters=torch.tensor(list(counters), device=cuda))


def _launch(st, picks, *, P, n, k, g, eos=None, init=False):
    from llx import kernels as K

    K.lookup_step(torch.tensor(picks, device=st["buf"].device), st["buf"][: P + n], st["len"], st["step_tok"], st["step_pos"], st["finished"],
                  st["counters"], P=P, n=n, k=k, g=g, eos_id=eos, init=init)


def _assert_state(st, want, tag):
    buf = st["buf"].cpu()
    L = want["len"][0]
    assert buf[:L].tolist() == want["seq"], tag
    assert (buf[L:] == PAD).all(), tag  # nothing behind the sequence was written, the slack behind cap included
    for name in ("len", "step_tok", "step_pos", "counters"):
        assert torch.equal(st[name].cpu(), torch.tensor(want[name], dtype=torch.int64)), (tag, name, st[name].tolist(), want[name])
    assert st["finished"].tolist() == want["finished"], tag


def _snapshot(st):
    return {k: v.clone() for k, v in st.items()}


@pytest.mark.parametrize("length", LENGTHS)
def test_step_equals_the_host_reference(cuda, length):
    from llx.sampling import lookup_draft

    seq = _tokens(length, 100 + length)
    P, n = max(1, length - 2), 12  # room for every accept count
    for g in (1, 3, 8):
        for k in (1, 2, 3):
            fed = [seq[-1]] + lookup_draft(seq, g, k)  # what the step before wrote
            for accept in range(k + 1):
                picks = _picks(fed, accept, k)
                st = _state(cuda, seq, fed, P=P, n=n, k=k)
                _launch(st, picks, P=P, n=n, k=k, g=g)
                want = _expect(seq, fed, picks, P=P, n=n, k=k, g=g)
                assert len(want["seq"]) == length + accept + 1
                _assert_state(st, want, (length, g, k, accept))


def test_first_step_after_the_prefill(cuda):
    """init: picks[0] is emitted, nothing is confirmed - whatever step_tok holds - and the first real step is drafted."""
    for length in (1, 5, 300):
        seq = _tokens(length, 7 + length)
        for k in (1, 3):
            for eos in (None, 2):
                stale = [seq[-1]] + [2] * k  # a picks row that "confirms" these must not count
                st = _state(cuda, seq, stale, P=length, n=6, k=k, counters=(0, 0))
                _launch(st, [2] * (k + 1), P=length, n=6, k=k, g=3, eos=eos, init=True)
                want = _expect(seq, stale, [2], P=length, n=6, k=k, g=3, eos=eos, init=True, counters=(0, 0))
                assert want["seq"] == seq + [2] and want["finished"] == [int(eos == 2)] and want["counters"] == [1, 0]
                _assert_state(st, want, (length, k, eos))


def test_eos_room_and_the_frozen_state(cuda):
    from llx.sampling import lookup_draft

    seq = _tokens(257, 11)
    k, g = 3, 3
    fed = [seq[-1]] + lookup_draft(seq, g, k)
    full = _picks(fed, k, k)  # confirms the whole draft: four tokens would be emitted
    cases = []
    for at in range(k + 1):  # eos at each emitted position: the output is cut behind it
        picks = list(full)
        picks[at] = 9
        fed_at = list(fed)
        if at < k:
            fed_at[1 + at] = 9  # (an eos that is a confirmed draft token)
        cases.append((fed_at, picks, 9, 12, at + 1, 1))
    rej = _picks(fed, 1, k)
    cases.append((fed, rej[:1] + [9] + rej[2:], 9, 12, 2, 1))  # eos is the first rejected position's own pick: emitted, ends the run
    cases.append((fed, rej[:2] + [9] + rej[3:], 9, 12, 2, 0))  # an eos behind the rejection is never emitted
    for room in (1, 2, 3, 4, 5):  # the room cuts the output; reaching P + n ends the run without the flag
        cases.append((fed, full, None, room, min(room, k + 1), 0))
    cases.append((fed[:2] + [9] + fed[3:], full[:1] + [9] + full[2:], 9, 1, 1, 0))  # a confirmed eos that falls behind the room
    for fed_c, picks, eos, room, emitted, fin in cases:
        P = 200
        n = len(seq) + room - P
        st = _state(cuda, seq, fed_c, P=P, n=n, k=k)
        _launch(st, picks, P=P, n=n, k=k, g=g, eos=eos)
        want = _expect(seq, fed_c, picks, P=P, n=n, k=k, g=g, eos=eos)
        assert len(want["seq"]) == len(seq) + emitted and want["finished"] == [fin], (picks, eos, room)
        _assert_state(st, want, (picks, eos, room))
        if fin or emitted == room:
            # frozen: a launch after the end - here one whose picks would confirm everything - changes no state tensor
            before = _snapshot(st)
            _launch(st, st["step_tok"][1:].tolist() + [1], P=P, n=n, k=k, g=g, eos=eos)
            for name, t in before.items():
                assert torch.equal(st[name], t), (name, picks, eos, room)
    # a state that arrives finished, or full, is not touched either
    for finished, room in ((1, 5), (0, 0)):
        P = 200
        n = len(seq) + room - P
        st = _state(cuda, seq, fed, P=P, n=n, k=k, finished=finished)
        before = _snapshot(st)
        _launch(st, full, P=P, n=n, k=k, g=g, eos=9)
        for name, t in before.items():
            assert torch.equal(st[name], t), (name, finished, room)


def test_large_token_ids(cuda):
    """Token ids up to the Llama-3 vocabulary's last one; ids that agree in their low 16 or 17 bits are different tokens."""
    from llx.sampling import lookup_draft

    ids = [128255, 128255 - 65536, 128255 - 256, 70000, 70000 - 65536]
    assert len(set(ids)) == 5 and max(ids) == 128255
    for length in (4, 257):
        seq = [ids[t] for t in _tokens(length, 31 + length)]
        for g, k in ((3, 3), (8, 2)):
            fed = [seq[-1]] + lookup_draft(seq, g, k)
            for accept in range(k + 1):
                picks = _picks(fed, accept, k, ids)
                st = _state(cuda, seq, fed, P=2, n=length + 10, k=k)
                _launch(st, picks, P=2, n=length + 10, k=k, g=g, eos=ids[0] if accept == k else None)
                _assert_state(st, _expect(seq, fed, picks, P=2, n=length + 10, k=k, g=g, eos=ids[0] if accept == k else None), (length, g, k, accept))


def test_wrapper_checks_its_tensors(cuda):
    from llx import kernels as K
    from llx._lib import LlxError

    st = _state(cuda, [1, 2, 3], [3, 3, 3], P=2, n=4, k=2)
    args = lambda **kw: {**dict(picks=torch.zeros(3, dtype=torch.int64, device=cuda), seq=st["buf"][:6], length=st["len"], step_tok=st["step_tok"],
                                step_pos=st["step_pos"], finished=st["finished"], counters=st["counters"]), **kw}
    for bad in (dict(picks=torch.zeros(2, dtype=torch.int64, device=cuda)), dict(seq=st["buf"][:5]), dict(step_tok=st["step_tok"][:2]),
                dict(finished=st["finished"].long()), dict(counters=st["counters"][:1]), dict(length=st["len"].cpu())):
        with pytest.raises(LlxError):
            K.lookup_step(**args(**bad), P=2, n=4, k=2, g=3)
    with pytest.raises(LlxError, match="k=4"):
        K.lookup_step(**args(picks=torch.zeros(5, dtype=torch.int64, device=cuda), step_tok=torch.zeros(5, dtype=torch.int64, device=cuda),
                             step_pos=torch.zeros(5, dtype=torch.int64, device=cuda)), P=2, n=4, k=4, g=3)
