"""CPU restatement of the 2-D deformable convolution (plain and modulated) for the tests: no kernel text, only torch operators.

A tap of a deformable group is one F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True) call in pixel coordinates:
zero padding there is exactly the operator's rule -- a corner outside the image contributes 0, so a sample at h <= -1, w <= -1, h >= H
or w >= W is 0 with a zero coordinate gradient.  The mask is multiplied in, the taps meet the weight in a grouped einsum, and every
gradient is autograd's.  tests/test_dcn2d_host.py pins this helper to the 3-D oracle at depth 1, to F.conv2d and to shifted taps.

Layouts: x [B, C, H, W], weight [K, C / group, kh, kw], offset [B, dg * 2 T, Ho, Wo] (channel 2 (i kw + j) = h, + 1 = w of tap (i, j)),
mask [B, dg * T, Ho, Wo] or None; input channel c uses deformable group c // (C // dg).
"""
import torch
import torch.nn.functional as F


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def out_size(H, W, kh, kw, stride, pad, dil):
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(pad), pair(dil)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def sample_positions(offset, H, W, kh, kw, stride, pad, dil, dg):
    """-> h, w [B, dg, T, Ho, Wo]: the sampling position of every (deformable group, tap, output position)."""
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(pad), pair(dil)
    B, _, Ho, Wo = offset.shape
    T = kh * kw
    off = offset.reshape(B, dg, T, 2, Ho, Wo)
    ti = (torch.arange(T) // kw).to(offset.dtype).view(1, 1, T, 1, 1)
    tj = (torch.arange(T) % kw).to(offset.dtype).view(1, 1, T, 1, 1)
    ys = (torch.arange(Ho) * sh - ph).to(offset.dtype).view(1, 1, 1, Ho, 1)
    xs = (torch.arange(Wo) * sw - pw).to(offset.dtype).view(1, 1, 1, 1, Wo)
    return ys + ti * dh + off[:, :, :, 0], xs + tj * dw + off[:, :, :, 1]


def deform_conv2d_ref(x, offset, mask, weight, bias, stride=1, pad=0, dil=1, group=1, dg=1):
    B, C, H, W = x.shape
    K, Cg, kh, kw = weight.shape
    assert H > 1 and W > 1 and C == Cg * group and K % group == 0 and C % dg == 0
    T, Cdg = kh * kw, C // dg
    Ho, Wo = out_size(H, W, kh, kw, stride, pad, dil)
    hpos, wpos = sample_positions(offset, H, W, kh, kw, stride, pad, dil, dg)
    taps = []
    for t in range(T):
        parts = []
        for g in range(dg):
            grid = torch.stack((2 * wpos[:, g, t] / (W - 1) - 1, 2 * hpos[:, g, t] / (H - 1) - 1), dim=-1)     # [B, Ho, Wo, (x, y)]
            s = F.grid_sample(x[:, g * Cdg:(g + 1) * Cdg], grid, mode='bilinear', padding_mode='zeros', align_corners=True)
            if mask is not None:
                s = s * mask[:, g * T + t].unsqueeze(1)
            parts.append(s)
        taps.append(torch.cat(parts, dim=1))
    col = torch.stack(taps, dim=2).reshape(B, group, Cg, T, Ho, Wo)
    out = torch.einsum('bgcthw,gkct->bgkhw', col, weight.reshape(group, K // group, Cg, T)).reshape(B, K, Ho, Wo)
    return out if bias is None else out + bias.view(1, K, 1, 1)


def outside_fractions(offset, H, W, kh, kw, stride, pad, dil, dg):
    """-> (fraction of (position, tap, group) samples with all four corners outside the image, fraction with some but not all outside)."""
    h, w = sample_positions(offset.double(), H, W, kh, kw, stride, pad, dil, dg)
    h0, w0 = torch.floor(h), torch.floor(w)
    inside = 0
    for jh in (0, 1):
        for jw in (0, 1):
            inside = inside + ((h0 + jh >= 0) & (h0 + jh <= H - 1) & (w0 + jw >= 0) & (w0 + jw <= W - 1)).long()
    # (a corner on an integer position carries weight 0 but still counts as a corner the kernel visits)
    return (inside == 0).double().mean().item(), ((inside > 0) & (inside < 4)).double().mean().item()
