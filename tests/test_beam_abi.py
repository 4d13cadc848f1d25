"""CPU: the beam-search entry points (csrc/beam.hip) are exported, declared in include/llx.h and bound in llx/_lib.py with the same number
of arguments; each validates its arguments before any launch (dummy pointers, a null stream: an error code and a message under the entry's
own name, no GPU needed); and generate() refuses what num_beams and audio= cannot run before anything is launched."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
P16 = P(16)


@pytest.mark.parametrize("name", ["llx_beam_rows", "llx_beam_merge", "llx_kv_reorder_rows"])
def test_entry_is_exported_declared_and_bound(name):
    from llx import _lib as L

    lib = L.load()
    assert hasattr(lib, name)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/llx.h"
    res, args = L.SIGNATURES[name]
    decl = [a.strip() for a in m.group(1).split(",")]
    assert res is ctypes.c_int and len(args) == len(decl)
    for ctype, text_arg in zip(args, decl):
        want = (ctypes.c_void_p if "*" in text_arg or "llx_stream_t" in text_arg else ctypes.c_int64 if "int64_t" in text_arg
                else ctypes.c_float if text_arg.startswith("float") else ctypes.c_int)
        assert ctype is want, (name, text_arg)


def _rows(lib, *, logits=P16, dtype=0, ld=1024, W=4, V=1000, score=P16, token=P16):
    return lib.llx_beam_rows(logits, dtype, ld, W, V, score, token, None)


def _merge(lib, *, W=4, n=8, hist_ld=8, bank_ld=8, eos=-1, lp=1.0, null=None):
    ptrs = [None if i == null else P16 for i in range(10)]
    return lib.llx_beam_merge(*ptrs[:6], hist_ld, ptrs[6], bank_ld, *ptrs[7:], W, n, eos, lp, 0, None)


def _reorder(lib, *, table=P16, n_caches=4, sb=8 * 64 * 128, sh=64 * 128, ss=128, parent=P16, W=4, KVH=8, length=5, Smax=64, hd=128):
    return lib.llx_kv_reorder_rows(table, n_caches, sb, sh, ss, parent, W, KVH, length, Smax, hd, None)


def test_beam_rows_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()
    err = lib.llx_last_error_string
    for kw, word in ((dict(W=1), b"W=1"), (dict(W=17), b"W=17"), (dict(V=4), b"V=4"), (dict(ld=999), b"stride"), (dict(dtype=2), b"dtype"),
                     (dict(logits=None), b"null"), (dict(score=None), b"null"), (dict(token=None), b"null"), (dict(logits=P(17)), b"aligned")):
        assert _rows(lib, **kw) == -1 and word in err() and err().startswith(b"llx_beam_rows:"), kw


def test_beam_merge_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()
    err = lib.llx_last_error_string
    for i in range(10):
        assert _merge(lib, null=i) == -1 and b"null" in err() and err().startswith(b"llx_beam_merge:"), i
    for kw, word in ((dict(W=1), b"W=1"), (dict(W=17), b"W=17"), (dict(n=0), b"n=0"), (dict(hist_ld=7), b"hist_ld=7"), (dict(bank_ld=7), b"bank_ld=7"),
                     (dict(eos=-2), b"eos_id"), (dict(lp=float("inf")), b"length_penalty"), (dict(lp=float("nan")), b"length_penalty")):
        assert _merge(lib, **kw) == -1 and word in err() and err().startswith(b"llx_beam_merge:"), kw


def test_kv_reorder_rows_rejects_before_launch():
    from llx import _lib as L

    lib = L.load()
    err = lib.llx_last_error_string
    for kw, word in ((dict(W=1), b"W=1"), (dict(W=17), b"W=17"), (dict(length=0), b"len=0"), (dict(length=65), b"len=65"),
                     (dict(table=None), b"pointer table"), (dict(table=P(20)), b"pointer table"), (dict(sb=8 * 64 * 128 + 4), b"strides"),
                     (dict(sh=64 * 128 + 2), b"strides"), (dict(ss=132), b"strides"), (dict(ss=64), b"strides"), (dict(parent=None), b"null"),
                     (dict(hd=64), b"head_dim"), (dict(n_caches=0), b"n_caches"), (dict(KVH=0), b"KVH")):
        assert _reorder(lib, **kw) == -1 and word in err() and err().startswith(b"llx_kv_reorder_rows:"), kw


def _text_model(batch):
    from modelling import Llama
    from oracle import ref as O
    from tests.util import to_model_config

    model = Llama(to_model_config(O.TINY._replace(num_layers=1, max_seq_len=64))).bfloat16()
    model.build_cache(inference=True, batch_size=batch)
    return model.eval()


def test_generate_refuses_what_beams_cannot_run():
    """The conditions of num_beams != 1 are checked before the device check, so a CPU model shows each of them."""
    from llx._lib import LlxError

    model = _text_model(4)
    prompt = torch.zeros(1, 40, dtype=torch.int64)
    for W in (0, 17, -2, 2.0):
        with pytest.raises(LlxError, match=r"num_beams=" + re.escape(repr(W))):
            model.generate(prompt, 8, num_beams=W)
    with pytest.raises(LlxError, match=r"num_beams=2 against a KV cache of batch 4.*batch_size=2"):
        model.generate(prompt, 8, num_beams=2)
    with pytest.raises(LlxError, match="num_beams=4 searches the continuations of one prompt"):
        model.generate(torch.zeros(4, 40, dtype=torch.int64), 8, num_beams=4)
    with pytest.raises(LlxError, match="num_beams=4.*prompt_lens"):
        model.generate(prompt, 8, num_beams=4, prompt_lens=[40])
    for kw, word in ((dict(temperature=0.7), "temperature=0.7"), (dict(top_k=5), "top_k=5"), (dict(top_p=0.9), "top_p=0.9")):
        with pytest.raises(LlxError, match="num_beams=4.*" + word):
            model.generate(prompt, 8, num_beams=4, **kw)
    with pytest.raises(LlxError, match="num_beams=4.*draft_tokens=2"):
        model.generate(prompt, 8, num_beams=4, draft_tokens=2)
    for lp in (float("inf"), float("nan"), "1", None):
        with pytest.raises(LlxError, match="length_penalty="):
            model.generate(prompt, 8, num_beams=4, length_penalty=lp)
    # everything beams ask for is in order: the next refusal is the device's
    with pytest.raises(LlxError, match="HIP device"):
        model.generate(prompt, 8, num_beams=4, length_penalty=0.5, eos_id=3)


def test_generate_refuses_what_audio_cannot_run():
    from llx._lib import LlxError
    from modelling import LlamaAudio
    from oracle import ref as O
    from tests.util import to_model_config

    with pytest.raises(LlxError, match="Llama or a LlamaAudio"):
        from llx.generate import generate

        generate(torch.nn.Linear(2, 2), torch.zeros(1, 4, dtype=torch.int64), 2)
    text = _text_model(1)
    prompt = torch.zeros(1, 20, dtype=torch.int64)
    clip = torch.zeros(1, 3200)
    with pytest.raises(LlxError, match="audio= needs a LlamaAudio"):
        text.generate(prompt, 4, audio=clip)
    model = LlamaAudio(to_model_config(O.TINY._replace(num_layers=1, max_seq_len=64))).bfloat16()
    model.build_cache(inference=True, batch_size=3)
    assert model.layers[0].attention.kv_cache.k_cache.shape[0] == 3  # build_cache forwards batch_size
    model.build_cache(inference=True)
    model.eval()
    assert model.audio_positions(3200) == 10 and model.audio_positions(160) == 1 and model.audio_positions(3360) == 11
    for bad in (torch.zeros(2, 3200), torch.zeros(3200), torch.zeros(1, 3200, dtype=torch.float64), torch.zeros(1, 100), [0.0] * 3200):
        with pytest.raises(LlxError, match=r"audio must be an fp32 tensor \[B, samples\]"):
            model.generate(bad, prompt, 4)
    with pytest.raises(LlxError, match="prefill_chunk=8 with audio"):
        model.generate(clip, prompt, 4, prefill_chunk=8)
    with pytest.raises(LlxError, match="draft_tokens=2 with audio"):
        model.generate(clip, prompt, 4, draft_tokens=2)
    with pytest.raises(LlxError, match="HIP device"):  # the clip is in order: the next refusal is the device's
        model.generate(clip, prompt, 34)
    with pytest.raises(LlxError, match="HIP device"):  # without a clip an audio model generates as a text model
        model.generate(None, prompt, 44)
