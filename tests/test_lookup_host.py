"""CPU: prompt-lookup drafting on the host - the reference functions lookup_draft / lookup_accept on cases worked out by hand, the
argument checks of the C entry point llx_lookup_step, and the conditions generate(draft_tokens=k) refuses before anything is launched."""
import ctypes

import pytest

P16 = ctypes.c_void_p(16)


def test_lookup_draft_by_hand():
    from llx.sampling import lookup_draft as draft

    assert draft([7], 3, 3) == [7, 7, 7]  # L = 1: no n-gram is shorter than the sequence
    # L = g: the 3-gram is skipped, [2, 1] has no earlier occurrence, the 1-gram [1] matches at j = 0 -> what followed it: 2, 1
    assert draft([1, 2, 1], 3, 2) == [2, 1]
    # L = g + 1: the 3-gram [6, 7, 5] may only sit at j = 0, where [5, 6, 7] stands; [7, 5] nowhere; [5] at j = 0
    assert draft([5, 6, 7, 5], 3, 3) == [6, 7, 5]
    # L = g + 1 with the g-gram matching at its only candidate j = 0 (it overlaps the tail: period 1)
    assert draft([4, 4, 4, 4], 3, 3) == [4, 4, 4]
    # a match at j = 0 only
    assert draft([9, 8, 3, 9, 8], 2, 2) == [3, 9]
    # two occurrences of [1, 2]: the later one (j = 3) wins -> 4, not 3
    assert draft([1, 2, 3, 1, 2, 4, 1, 2], 2, 1) == [4]
    assert draft([1, 2, 3, 1, 2, 4, 1, 2], 2, 3) == [4, 1, 2]
    # the 3-gram [1, 2, 3] occurs at j = 0 only, the 1-gram [3] more recently at index 5: the longer n-gram wins
    assert draft([1, 2, 3, 7, 9, 3, 5, 1, 2, 3], 3, 1) == [7]
    assert draft([1, 2, 3, 7, 9, 3, 5, 1, 2, 3], 1, 1) == [5]
    assert draft([1, 2, 3, 7, 9, 3, 5, 1, 2, 3], 8, 2) == [7, 9]  # n-grams of 8 .. 4 tokens have no match
    # a match that overlaps the tail continues periodically: period 1 ...
    assert draft([5, 36, 36], 3, 3) == [36, 36, 36]
    # ... and period 2: [1, 2] at j = 1, src = 3 -> seq[3], seq[4], then the draft's own first token
    assert draft([0, 1, 2, 1, 2], 2, 3) == [1, 2, 1]
    # no match at any length: the last token is repeated
    assert draft([1, 2, 3], 3, 2) == [3, 3]
    assert draft([1, 2, 3], 1, 1) == [3]


def test_lookup_accept_by_hand():
    from llx.sampling import lookup_accept as accept

    fed = [10, 11, 12, 13]
    assert accept(fed, [99, 12, 13, 50], 3, None, 9) == ([99], False)  # nothing confirmed: the model's own token alone
    assert accept(fed, [11, 99, 13, 50], 3, None, 9) == ([11, 99], False)
    assert accept(fed, [11, 12, 99, 50], 3, None, 9) == ([11, 12, 99], False)
    assert accept(fed, [11, 12, 13, 50], 3, None, 9) == ([11, 12, 13, 50], False)
    assert accept(fed, [11, 12, 13, 50], 3, -1, 9) == ([11, 12, 13, 50], False)
    assert accept([1, 2], [2, 3], 1, None, 9) == ([2, 3], False)
    assert accept([1, 2, 2], [2, 3, 2], 2, None, 9) == ([2, 3], False)  # a later agreement after a rejection does not count
    # eos at an accepted position, at the first rejected one, and behind it (not emitted, so not seen)
    assert accept(fed, [11, 12, 13, 50], 3, 12, 9) == ([11, 12], True)
    assert accept(fed, [11, 77, 13, 50], 3, 77, 9) == ([11, 77], True)
    assert accept(fed, [99, 77, 13, 50], 3, 77, 9) == ([99], False)
    assert accept(fed, [11, 12, 13, 50], 3, 50, 9) == ([11, 12, 13, 50], True)
    # room
    assert accept(fed, [11, 12, 13, 50], 3, None, 1) == ([11], False)
    assert accept(fed, [11, 12, 13, 50], 3, None, 2) == ([11, 12], False)
    assert accept(fed, [11, 12, 13, 50], 3, 12, 1) == ([11], False)  # the eos is cut off with the room: the length ends the run
    assert accept(fed, [11, 12, 13, 50], 3, 12, 2) == ([11, 12], True)
    assert accept(fed, [99, 12, 13, 50], 3, None, 2) == ([99], False)


def _step(lib, *, picks=P16, seq=P16, cap=64, length=P16, step_tok=P16, step_pos=P16, finished=P16, counters=P16, P=8, n=8, k=3, g=3, eos=-1,
          init=0):
    return lib.llx_lookup_step(picks, seq, cap, length, step_tok, step_pos, finished, counters, P, n, k, g, eos, init, None)


def test_lookup_entry_point_rejects_bad_arguments():
    from llx import _lib as L

    lib = L.load()
    for name in ("picks", "seq", "length", "step_tok", "step_pos", "finished", "counters"):
        assert _step(lib, **{name: None}) == -1 and b"null pointer" in lib.llx_last_error_string(), name
    for k in (0, 4, -1):
        assert _step(lib, k=k) == -1 and b"k=" in lib.llx_last_error_string() and b"1..3" in lib.llx_last_error_string()
    for g in (0, 9):
        assert _step(lib, g=g) == -1 and b"g=" in lib.llx_last_error_string() and b"1..8" in lib.llx_last_error_string()
    assert _step(lib, cap=15) == -1 and b"cap=15" in lib.llx_last_error_string() and b"P + n" in lib.llx_last_error_string()
    assert _step(lib, P=0) == -1 and b"P=0" in lib.llx_last_error_string()
    assert _step(lib, n=0) == -1 and b"n=0" in lib.llx_last_error_string()
    assert _step(lib, eos=-2) == -1 and b"eos_id" in lib.llx_last_error_string()
    assert b"llx_lookup_step" in lib.llx_last_error_string()


def test_generate_refuses_what_drafting_cannot_run():
    """The conditions of draft_tokens != 0 are checked before the device check, so a CPU model shows each of them."""
    import torch

    from llx._lib import LlxError
    from modelling import Llama
    from oracle import ref as O
    from tests.util import to_model_config

    cfg = O.TINY._replace(num_layers=1, max_seq_len=64)
    model = Llama(to_model_config(cfg)).bfloat16()
    model.build_cache(inference=True)
    model.eval()
    prompt = torch.zeros(1, 40, dtype=torch.int64)
    with pytest.raises(LlxError, match="temperature == 0"):
        model.generate(prompt, 8, draft_tokens=2, temperature=0.7)
    with pytest.raises(LlxError, match="draft_tokens=4"):
        model.generate(prompt, 8, draft_tokens=4)
    with pytest.raises(LlxError, match="draft_tokens=-1"):
        model.generate(prompt, 8, draft_tokens=-1)
    with pytest.raises(LlxError, match="draft_ngram=0"):
        model.generate(prompt, 8, draft_tokens=2, draft_ngram=0)
    with pytest.raises(LlxError, match="draft_ngram=9"):
        model.generate(prompt, 8, draft_tokens=2, draft_ngram=9)
    with pytest.raises(LlxError, match=r"\+ draft_tokens \(3\) exceeds max_seq_len"):
        model.generate(prompt, 64 - 40 - 3 + 1, draft_tokens=3)
    with pytest.raises(LlxError, match="one sequence"):
        model.generate(prompt, 8, draft_tokens=2, prompt_lens=[39])
    # P + n + k == max_seq_len passes the drafting checks: the next refusal is the device's
    with pytest.raises(LlxError, match="HIP device"):
        model.generate(prompt, 64 - 40 - 3, draft_tokens=3)
    model.build_cache(inference=True, batch_size=2)
    with pytest.raises(LlxError, match="one sequence"):
        model.generate(torch.zeros(2, 40, dtype=torch.int64), 8, draft_tokens=2)
