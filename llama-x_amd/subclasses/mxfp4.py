"""OCP MXFP4 weight-only linear weight as a tensor subclass, HIP-backed (csrc/mxfp4.hip).

A weight [N, K] (K % 32 == 0) is stored as ``packed`` uint8 [N, K/2] (byte j: element 2j in bits 0-3, element 2j+1 in bits 4-7; a code
is sign << 3 | e2m1, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6) and ``scale`` uint8 [N, K/32] (the biased exponent b of a block of 32
consecutive k; block scale 2^(b - 127)): 4.25 bits per weight.  The subclass reports shape (N, K) and dtype bf16, and every linear on it
behaves as a bf16 linear whose weight is ``dequantize()``: the decode path streams the packed rows (llx_gemv_mxfp4), every other path
multiplies by a transient bf16 image that is never kept.
"""
import torch
import torch.nn.functional as F
from torch import Tensor

from llx import _lib as L
from llx import kernels as K

aten = torch.ops.aten

BLOCK = 32
_MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4(x: Tensor) -> tuple[Tensor, Tensor]:
    """(packed, scale) of x [N, K], bf16 or fp32, computed in fp32: per block amax = max |x|; b = 127 when amax == 0, else
    e = clamp(floor(log2 amax) - 2, -125, 125), b = e + 127; |x| * 2^-e rounded to the nearest magnitude, ties to the code with mantissa
    bit 0, above 6 saturated; the sign bit is the input's.  Device tensors run llx_quantize_mxfp4; the host form below is bit-identical
    (the scripts quantise before .cuda())."""
    if x.dim() != 2 or x.shape[1] % BLOCK != 0 or x.shape[1] == 0:
        raise L.LlxError(f"quantize_mxfp4: a [N, K] matrix with K a multiple of {BLOCK} is required, got {tuple(x.shape)}")
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise L.LlxError(f"quantize_mxfp4: unsupported dtype {x.dtype} (bf16 or fp32)")
    if x.is_cuda:
        return K.quantize_mxfp4(x)
    N, Kd = x.shape
    blk = x.to(torch.float32).contiguous().view(N, Kd // BLOCK, BLOCK)
    mag = blk.abs()
    amax = mag.amax(dim=-1)
    # floor(log2 amax) = the exponent field of a normal fp32; a denormal amax falls below the clamp either way
    e = (((amax.view(torch.int32) >> 23) & 0xFF) - 129).clamp(-125, 125)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    inv = ((127 - e) << 23).view(torch.float32)  # 2^-e, a normal fp32: the product below is exact
    v = mag * inv.unsqueeze(-1)
    code = ((v > 0.25).to(torch.uint8) + (v >= 0.75).to(torch.uint8) + (v > 1.25).to(torch.uint8) + (v >= 1.75).to(torch.uint8)
            + (v > 2.5).to(torch.uint8) + (v >= 3.5).to(torch.uint8) + (v > 5.0).to(torch.uint8))
    code = code | ((blk.view(torch.int32) < 0).to(torch.uint8) << 3)
    code = code.view(N, Kd // 2, 2)
    packed = code[..., 0] | (code[..., 1] << 4)
    return packed.contiguous(), (e + 127).to(torch.uint8)


def dequantize_mxfp4(packed: Tensor, scale: Tensor) -> Tensor:
    """The bf16 image [N, K]: magnitude * 2^(b - 127), exact."""
    if packed.is_cuda:
        return K.dequantize_mxfp4(packed, scale)
    N, Kd = packed.shape[0], packed.shape[1] * 2
    code = torch.stack((packed & 0xF, packed >> 4), dim=-1).view(N, Kd).to(torch.int64)
    val = torch.tensor(_MAGNITUDES, dtype=torch.float32)[code & 7]
    val = torch.where((code & 8) != 0, -val, val)
    blk_scale = (scale.to(torch.int32) << 23).view(torch.float32)
    return (val.view(N, Kd // BLOCK, BLOCK) * blk_scale.unsqueeze(-1)).view(N, Kd).to(torch.bfloat16)


class MXFP4LinearWeight(Tensor):
    @staticmethod
    @torch._dynamo.disable
    def __new__(cls, packed: Tensor, scale: Tensor):
        # a wrapper subclass: reports the logical shape (N, K) and bf16, the dtype of its image
        return Tensor._make_wrapper_subclass(cls, (packed.shape[0], packed.shape[1] * 2), dtype=torch.bfloat16, device=packed.device)

    @torch._dynamo.disable
    def __init__(self, packed: Tensor, scale: Tensor):
        assert packed.dtype is torch.uint8 and scale.dtype is torch.uint8
        assert packed.ndim == 2 and scale.ndim == 2
        assert packed.shape[1] % (BLOCK // 2) == 0 and tuple(scale.shape) == (packed.shape[0], packed.shape[1] * 2 // BLOCK)
        self.packed = packed
        self.scale = scale

    # ---- serialisation hooks (state_dict / torch.save round trip)
    def __tensor_flatten__(self):
        return ["packed", "scale"], []

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size=None, outer_stride=None):
        return cls(tensor_data_dict["packed"], tensor_data_dict["scale"])

    @classmethod
    def from_float(cls, tensor: Tensor):
        if tensor.dim() != 2 or tensor.shape[1] % BLOCK != 0:
            raise L.LlxError(f"MXFP4LinearWeight: in_features={tensor.shape[-1]} must be a multiple of {BLOCK}")
        if not bool(torch.isfinite(tensor).all()):  # one host check: this runs at model-surgery time
            raise L.LlxError("MXFP4LinearWeight: non-finite weight")
        return cls(*quantize_mxfp4(tensor))

    def dequantize(self):
        return dequantize_mxfp4(self.packed, self.scale)

    def __repr__(self):
        return f"{self.__class__.__name__}(shape={tuple(self.shape)}, dtype={self.dtype}, device={self.device}, requires_grad={self.requires_grad})"

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear:
            return _MXFP4Linear.apply(*args, **kwargs)
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs):
        handler = _DISPATCH.get(func)
        if handler is None:
            raise NotImplementedError(f"{cls.__name__} dispatch: attempting to run {func}, this is not supported")
        return handler(cls, func, args, kwargs)


def _rewrap(cls, func, args, kwargs):
    w = args[0]
    return cls(func(w.packed, *args[1:], **kwargs), func(w.scale, *args[1:], **kwargs))


def _to_copy(cls, func, args, kwargs):
    w = args[0]
    device = kwargs.get("device", None)  # (a dtype is not applied: the stored bytes are the format)
    return cls(w.packed.to(device=device), w.scale.to(device=device))


def _copy_(cls, func, args, kwargs):
    dst, src = args[0], args[1]
    if isinstance(dst, cls) and isinstance(src, cls):
        dst.packed.copy_(src.packed)
        dst.scale.copy_(src.scale)
    elif isinstance(dst, cls):  # float -> MXFP4: re-quantise
        fresh = cls.from_float(src)
        dst.packed.copy_(fresh.packed)
        dst.scale.copy_(fresh.scale)
    else:  # MXFP4 -> float
        dst.copy_(src.dequantize())
    return dst


_DISPATCH = {
    aten.detach.default: _rewrap,
    aten.clone.default: _rewrap,
    aten._to_copy.default: _to_copy,
    aten.copy_.default: _copy_,
}


class _MXFP4Linear(torch.autograd.Function):
    """F.linear on an MXFP4LinearWeight: the bf16 product on a transient image of the weight; no weight gradient, bias added after."""

    @staticmethod
    def forward(ctx, input: Tensor, weight: MXFP4LinearWeight, bias: Tensor | None = None):
        L.require_cuda(input)
        ctx.weight = weight
        x2 = K._rows2d(input)
        out = K.gemm_nt(x2, K.dequantize_mxfp4(weight.packed, weight.scale)).view(*input.shape[:-1], -1)
        if bias is not None:
            out = out + bias
        return out

    @staticmethod
    def backward(ctx, grad_output: Tensor):
        w: MXFP4LinearWeight = ctx.weight
        grad_input = None
        if ctx.needs_input_grad[0]:
            wt = K.dequantize_mxfp4(w.packed, w.scale, transpose=True)
            grad_input = K.gemm_nt(K._rows2d(grad_output), wt).view(*grad_output.shape[:-1], w.shape[1])
        grad_bias = None
        if len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2]:
            grad_bias = grad_output.reshape(-1, w.shape[0]).sum(0)
        return grad_input, None, grad_bias
