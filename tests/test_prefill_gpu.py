"""GPU: KV-cache prefill through the public model API (Llama.forward(x, input_pos=...)) on the tiny configuration, max_seq_len 512:
chunked prefill against the oracle's restatement of the reference's cached path, the routing of _run_dense (masks broadcast over
heads run on llx_attn_mask_fwd, per-head masks on llx_attn_dense_fwd), and a prefill chunk captured in a graph."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref as O
from tests.util import _close, bf16_params, to_model_config

pytestmark = pytest.mark.gpu

CFG = O.TINY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def setup(cuda):
    from modelling import Llama

    pb, pf = bf16_params(O.init_params(CFG))
    model = Llama(to_model_config(CFG)).bfloat16()
    model.load_state_dict(pb, strict=False)
    model.build_cache(inference=True)
    model = model.to(cuda).eval()
    tokens = O.randint("prefill_tokens", (1, 501), 0, CFG.vocab_size)
    return model, pf, tokens


def _reset(model):
    for layer in model.layers:
        layer.attention.kv_cache.k_cache.zero_()
        layer.attention.kv_cache.v_cache.zero_()


CALLS = ((0, 200), (200, 500), (500, 501))  # two prefill chunks, then one decode step


def test_chunked_prefill_against_the_oracle(setup, cuda):
    """Test 7: input_pos = arange(0, 200), arange(200, 500), then one decode step at 500, against O.llama_forward_cached with the same
    three calls (it restates the reference's quirk that RoPE rows restart at 0 on every call).  Logits within the 3 % bar of
    test_kv_cache_prefill_and_decode; the caches afterwards equal the oracle's at rows 0..500 within the 2 % bar the decode tests use
    for cache rows written by the model, rows 501..511 still zero."""
    model, pf, tokens = setup
    _reset(model)
    cache = O.new_cache(CFG)
    with torch.no_grad():
        for lo, hi in CALLS:
            pos = torch.arange(lo, hi)
            got = model(tokens[:, lo:hi].to(cuda), input_pos=pos.to(cuda))
            want = O.llama_forward_cached(tokens[:, lo:hi], pf, CFG, cache, pos)
            _close(got.float().cpu(), want, 0.03, f"logits of the call at positions {lo}..{hi - 1}")
    for i, layer in enumerate(model.layers):
        for name, dev, ref in (("k", layer.attention.kv_cache.k_cache, cache[i][0]), ("v", layer.attention.kv_cache.v_cache, cache[i][1])):
            _close(dev[:, :, :501].float().cpu(), ref[:, :, :501], 0.02, f"layer {i} {name} cache rows 0..500")
            assert not bool(dev[:, :, 501:].any()), f"layer {i} {name} cache rows 501..511 were written"


def test_routing(setup, cuda, monkeypatch):
    """Test 8: with K.attn_dense_fwd patched to raise, the two prefill calls and a no-grad layer(x, rope, mask=dense prefix-LM) at
    S 384 still succeed (they run on the mask-driven MFMA kernel); a per-head mask [1, H, S, S] reaches the patched function."""
    from llx import kernels as K

    model, pf, tokens = setup

    class Reached(Exception):
        pass

    def boom(*a, **kw):
        raise Reached()

    monkeypatch.setattr(K, "attn_dense_fwd", boom)
    _reset(model)
    with torch.no_grad():
        for lo, hi in CALLS[:2]:
            out = model(tokens[:, lo:hi].to(cuda), input_pos=torch.arange(lo, hi, device=cuda))
            assert bool(torch.isfinite(out).all())
        layer = model.layers[0]
        kvc = layer.attention.kv_cache
        layer.attention.kv_cache = None
        try:
            hid = O.randn("hidden1", (1, 384, 512), 0.5).bfloat16()
            dense = O.prefix_lm_mask(384, [128])
            out = layer(hid.to(cuda), model.rope[:384], mask=dense.to(cuda))
            want = O.layer(hid.float(), pf, 0, CFG, O.rope_table(CFG)[:384], dense)
            _close(out.float().cpu(), want, 0.03, "layer with dense prefix-LM mask")
            per_head = dense.expand(1, CFG.num_heads, 384, 384).contiguous()
            with pytest.raises(Reached):
                layer(hid.to(cuda), model.rope[:384], mask=per_head.to(cuda))
        finally:
            layer.attention.kv_cache = kvc


_GRAPH_SCRIPT = r"""
import sys, torch
root = sys.argv[1]
sys.path[:0] = [root + "/llama-x_amd", root]
from oracle import ref as O
from tests.util import bf16_params, to_model_config
from modelling import Llama
CFG = O.TINY
dev = torch.device("cuda:0")
pb, _ = bf16_params(O.init_params(CFG))
model = Llama(to_model_config(CFG)).bfloat16()
model.load_state_dict(pb, strict=False)
model.build_cache(inference=True)
model = model.to(dev).eval()
tokens = O.randint("prefill_tokens", (1, 501), 0, CFG.vocab_size).to(dev)
caches = [c for l in model.layers for c in (l.attention.kv_cache.k_cache, l.attention.kv_cache.v_cache)]
with torch.no_grad():
    model(tokens[:, :200], input_pos=torch.arange(0, 200, device=dev))
    saved = [c.clone() for c in caches]
    tok, pos = tokens[:, 200:500].contiguous(), torch.arange(200, 500, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = model(tok, input_pos=pos)
    torch.cuda.current_stream().wait_stream(side)
    eager_caches = [c.clone() for c in caches]
    for c, s in zip(caches, saved):
        c.copy_(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits = model(tok, input_pos=pos)
    for c, s in zip(caches, saved):
        c.copy_(s)
    logits.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert bool(eager.abs().max() > 0)
    assert torch.equal(logits, eager), "graph replay of a prefill chunk differs from the eager call"
    assert all(torch.equal(a, b) for a, b in zip(caches, eager_caches)), "caches after the replay differ from the eager call's"
print("graph ok")
"""


def test_prefill_chunk_in_a_graph(cuda):
    """Test 9: the 300-token chunk captured in a torch.cuda.graph in a fresh child process (its default setup) and replayed once
    gives the eager logits bit for bit: the prefill path makes no host synchronisation."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "graph ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
