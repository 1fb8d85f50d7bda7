"""SwinIR's (shifted-)window attention between a block's qkv and proj Linears as one call, on the kernels of
ssl_amd/csrc/ssg_winattn.hip (include/ssg_hip.h section (Z)).

    out = window_attention(qkv, bias_table, num_heads, window_size=8, shift_size=0, scale=None)

`qkv` is (B, H, W, 3 C): the block's qkv Linear applied to the UNPARTITIONED token grid (a Linear acts per token, so it
commutes with the roll and the partition); `bias_table` the module's ((2 ws - 1)^2, heads) parameter; `out` is
(B, H, W, C), what proj consumes.  The cyclic shift, the window partition, the qkv permute, q * scale, q k^T, the
relative-position bias, the shift mask, the softmax, attn v, the merge and the reverse shift of
GAN-Based-SR/basicsr/archs/swinir_arch.py happen inside.  Once differentiable, with gradients for qkv and bias_table.

The native domain ("Which calls take the kernels"): `_gpu.native(qkv, bias_table)` (the switch of
set_native_criteria is on; fp32 tensors on one GPU), both contiguous, window 8, head_dim <= 32, H and W multiples of 8,
0 <= shift < 8.  Every other call -- CPU, fp64, half, another window, head_dim > 32 -- takes `torch_route`: the
reference's operations in the reference's order and so the reference's bits.  A call outside both (a shape the
reference itself cannot partition) raises as torch does.

The forward saves qkv and the table only: the backward recomputes the softmax, so no (windows, heads, 64, 64) tensor
exists at any time.  Neither call allocates inside the library, copies or synchronises, so both may be captured.
"""
import torch

from . import _gpu, _lib

__all__ = ["window_attention", "torch_route", "is_native", "relative_position_index", "shift_mask"]

WINDOW = 8
MAX_HEAD_DIM = 32


# ---- the seam between this module and the library (tests count and replace it) ----
def _library():
    return _lib.lib()


def relative_position_index(window_size):
    """The (ws^2, ws^2) table row of each (query, key) pair: (iy_i - iy_j + ws - 1)(2 ws - 1) + (ix_i - ix_j + ws - 1)."""
    ws = window_size
    iy, ix = torch.arange(ws * ws) // ws, torch.arange(ws * ws) % ws
    return (iy[:, None] - iy[None, :] + ws - 1) * (2 * ws - 1) + (ix[:, None] - ix[None, :] + ws - 1)


def _windows(x, ws):
    """(B, H, W, ...) -> (B nW, ws ws, ...) by the reference's view, permute and copy."""
    b, h, w = x.shape[:3]
    rest = x.shape[3:]
    x = x.view(b, h // ws, ws, w // ws, ws, *rest)
    return x.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).contiguous().view(-1, ws * ws, *rest)


def shift_mask(h, w, window_size, shift_size):
    """The reference's calculate_mask: (nW, ws^2, ws^2) of 0 and -100 for an (h, w) grid rolled by -shift."""
    ws = window_size
    regions = torch.zeros((1, h, w, 1))
    bands = (slice(0, -ws), slice(-ws, -shift_size), slice(-shift_size, None))
    count = 0
    for rows in bands:
        for cols in bands:
            regions[:, rows, cols, :] = count
            count += 1
    labels = _windows(regions, ws).view(-1, ws * ws)
    diff = labels.unsqueeze(1) - labels.unsqueeze(2)
    return diff.masked_fill(diff != 0, float(-100.0)).masked_fill(diff == 0, float(0.0))


def torch_route(qkv, bias_table, num_heads, window_size=WINDOW, shift_size=0, scale=None, mask=None, index=None,
                attn_drop=None):
    """The reference's lines on (B, H, W, 3 C): roll, partition, permute, q * scale, q k^T, + bias, + mask, softmax,
    (dropout,) attn v, transpose, merge, roll back.  mask / index: the module's buffers where the caller has them (the
    same values are built here otherwise)."""
    b, h, w, c3 = qkv.shape
    ws, c = window_size, c3 // 3
    d = c // num_heads
    scale = d ** -0.5 if scale is None else scale
    if shift_size > 0:
        qkv = torch.roll(qkv, shifts=(-shift_size, -shift_size), dims=(1, 2))
    win = _windows(qkv, ws)                                              # (B nW, n, 3 C)
    b_, n = win.shape[:2]
    parts = win.reshape(b_, n, 3, num_heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = parts[0], parts[1], parts[2]
    q = q * scale
    attn = q @ k.transpose(-2, -1)
    if index is None:
        index = relative_position_index(ws).to(bias_table.device)
    bias = bias_table[index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if shift_size > 0:
        if mask is None:
            mask = shift_mask(h, w, ws, shift_size).to(device=qkv.device, dtype=qkv.dtype)
        nw = mask.shape[0]
        attn = attn.view(b_ // nw, nw, num_heads, n, n) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, num_heads, n, n)
    attn = torch.softmax(attn, dim=-1)
    if attn_drop is not None:
        attn = attn_drop(attn)
    x = (attn @ v).transpose(1, 2).reshape(b_, n, c)
    x = x.view(b, h // ws, w // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5).contiguous().view(b, h, w, c)
    if shift_size > 0:
        x = torch.roll(x, shifts=(shift_size, shift_size), dims=(1, 2))
    return x


def is_native(qkv, bias_table, num_heads, window_size=WINDOW, shift_size=0):
    """Whether window_attention hands this call to the kernels."""
    if not _gpu.native(qkv, bias_table):
        return False
    if qkv.dim() != 4 or bias_table.dim() != 2 or window_size != WINDOW or num_heads < 1:
        return False
    b, h, w, c3 = qkv.shape
    if b < 1 or h < 1 or w < 1 or c3 % (3 * num_heads) or h % WINDOW or w % WINDOW:
        return False
    d = c3 // (3 * num_heads)
    return (1 <= d <= MAX_HEAD_DIM and 0 <= shift_size < WINDOW and qkv.is_contiguous() and bias_table.is_contiguous()
            and tuple(bias_table.shape) == ((2 * WINDOW - 1) ** 2, num_heads))


def _shape(qkv, num_heads):
    b, h, w, c3 = qkv.shape
    return b, h, w, num_heads, c3 // (3 * num_heads)


class _WindowAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias_table, num_heads, shift, scale):
        qkv, bias_table = qkv.detach(), bias_table.detach()
        b, h, w, heads, d = _shape(qkv, num_heads)
        with _gpu.on(qkv.device):
            out = torch.empty((b, h, w, heads * d), dtype=torch.float32, device=qkv.device)
        _gpu.launch(qkv.device, _library().ssg_winattn_forward, qkv.data_ptr(), bias_table.data_ptr(), out.data_ptr(),
                    b, h, w, heads, d, shift, scale)
        ctx.save_for_backward(qkv, bias_table)
        ctx.args = (num_heads, shift, scale)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        qkv, bias_table = ctx.saved_tensors
        num_heads, shift, scale = ctx.args
        if not _gpu.readable(dout) or dout.device != qkv.device:
            raise RuntimeError("ssl_amd.winattn: the gradient of a native call must be an fp32 tensor on its GPU")
        dout = dout.contiguous()
        b, h, w, heads, d = _shape(qkv, num_heads)
        L = _library()
        want_table = ctx.needs_input_grad[1]
        with _gpu.on(qkv.device):
            dqkv = torch.empty_like(qkv)
            dtable = torch.empty_like(bias_table) if want_table else None
            ws, ws_bytes = _gpu.workspace(L.ssg_winattn_workspace_bytes(b, h, w, heads, d) if want_table else 0,
                                          qkv.device)
        _gpu.launch(qkv.device, L.ssg_winattn_backward, qkv.data_ptr(), bias_table.data_ptr(), dout.data_ptr(),
                    dqkv.data_ptr(), _gpu.ptr(dtable), ws.data_ptr(), ws_bytes, b, h, w, heads, d, shift, scale)
        return dqkv if ctx.needs_input_grad[0] else None, dtable, None, None, None


def window_attention(qkv, bias_table, num_heads, window_size=WINDOW, shift_size=0, scale=None):
    """(B, H, W, C) from qkv (B, H, W, 3 C) and the ((2 ws - 1)^2, heads) bias table; see the module's text."""
    if is_native(qkv, bias_table, num_heads, window_size, shift_size):
        d = qkv.shape[3] // (3 * num_heads)
        return _WindowAttention.apply(qkv, bias_table, num_heads, int(shift_size),
                                      float(d ** -0.5 if scale is None else scale))
    return torch_route(qkv, bias_table, num_heads, window_size, shift_size, scale)
