"""The two post-processing filters of the post_process block restated in torch on the CPU, from the definitions alone (DESIGN.md section 7;
include/dpf_hip.h): fp64 by default -- the oracle of tests/test_gpu_postprocess.py -- and, with dtype=torch.float32 (the *_fp32 names), the
straightforward fp32 evaluation whose own distance from fp64 sets the bars there.  Nothing here follows the kernels: window sums are
differences of zero-padded cumulative sums of the raw quantities, the bilateral filter is a loop over taps of shifted images.

    luminance(guide_rgb)                                I = 0.299 R + 0.587 G + 0.114 B, R = x_0 * 0.229 + 0.485 ...
    guided_filter(p, guide_rgb, r, eps)                 a = cov(I, p) / (var(I) + eps), b = mean p - a mean I, q = mean(a) I + mean(b)
    joint_bilateral_filter(p, guide_rgb, r, ss, sc)     q(x) = sum w_s w_c p(y) / sum w_s w_c over the clipped window
"""
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # written out: the test of the package's constants compares against these
LUMA = (0.299, 0.587, 0.114)


def luminance(guide_rgb, dtype=torch.float64):
    g = guide_rgb.to(dtype)
    out = torch.zeros_like(g[:, 0])
    for c in range(3):
        out = out + LUMA[c] * (g[:, c] * STD[c] + MEAN[c])
    return out                                                   # [B, H, W]


def box_sum(x, r):
    """Sum over the (2r+1)^2 window clipped at the border, for the last two axes of x."""
    H, W = x.shape[-2:]
    c = torch.zeros(x.shape[:-2] + (H + 1, W + 1), dtype=x.dtype)
    c[..., 1:, 1:] = x.cumsum(-2).cumsum(-1)
    y0 = (torch.arange(H) - r).clamp(min=0)
    y1 = (torch.arange(H) + r + 1).clamp(max=H)
    x0 = (torch.arange(W) - r).clamp(min=0)
    x1 = (torch.arange(W) + r + 1).clamp(max=W)
    return c[..., y1[:, None], x1[None, :]] - c[..., y0[:, None], x1[None, :]] - c[..., y1[:, None], x0[None, :]] + c[..., y0[:, None], x0[None, :]]


def window_count(H, W, r, dtype=torch.float64):
    ny = (torch.arange(H) + r).clamp(max=H - 1) - (torch.arange(H) - r).clamp(min=0) + 1
    nx = (torch.arange(W) + r).clamp(max=W - 1) - (torch.arange(W) - r).clamp(min=0) + 1
    return (ny[:, None] * nx[None, :]).to(dtype)


def guided_from_plane(p, I, r, eps, dtype=torch.float64):
    """p [B, n, H, W], I [B, H, W] -> q [B, n, H, W]."""
    p, I = p.to(dtype), I.to(dtype).unsqueeze(1)
    N = window_count(p.shape[-2], p.shape[-1], r, dtype)
    mean = lambda x: box_sum(x, r) / N
    mI, mp = mean(I), mean(p)
    a = (mean(I * p) - mI * mp) / (mean(I * I) - mI * mI + eps)
    b = mp - a * mI
    return mean(a) * I + mean(b)


def guided_filter(p, guide_rgb, r, eps, dtype=torch.float64):
    return guided_from_plane(p, luminance(guide_rgb, dtype), r, eps, dtype)


def bilateral_from_plane(p, I, r, sigma_space, sigma_color, dtype=torch.float64):
    p, I = p.to(dtype), I.to(dtype).unsqueeze(1)
    H, W = p.shape[-2:]
    num, den = torch.zeros_like(p), torch.zeros_like(p)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            # the pixels x for which the tap y = x + (dy, dx) lies inside the image
            ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if ya >= yb or xa >= xb:
                continue
            ws = torch.exp(torch.tensor(-(dy * dy + dx * dx) / (2.0 * sigma_space * sigma_space), dtype=dtype))
            dI = I[..., ya:yb, xa:xb] - I[..., ya + dy:yb + dy, xa + dx:xb + dx]
            w = ws * torch.exp(-(dI * dI) / (2.0 * sigma_color * sigma_color))
            num[..., ya:yb, xa:xb] += w * p[..., ya + dy:yb + dy, xa + dx:xb + dx]
            den[..., ya:yb, xa:xb] += w
    return num / den


def joint_bilateral_filter(p, guide_rgb, r, sigma_space, sigma_color, dtype=torch.float64):
    return bilateral_from_plane(p, luminance(guide_rgb, dtype), r, sigma_space, sigma_color, dtype)


def guided_filter_fp32(p, guide_rgb, r, eps):
    return guided_filter(p, guide_rgb, r, eps, dtype=torch.float32)


def joint_bilateral_filter_fp32(p, guide_rgb, r, sigma_space, sigma_color):
    return joint_bilateral_filter(p, guide_rgb, r, sigma_space, sigma_color, dtype=torch.float32)


def to_guide(I01):
    """An RGB guide [B, 3, H, W] in normalised form whose luminance is the grey image I01 [B, H, W] (R = G = B = I01; the luma weights sum
    to 1), fp64."""
    I01 = I01.double()
    return torch.stack([(I01 - MEAN[c]) / STD[c] for c in range(3)], dim=1)


def scene(B, n, H, W, seed, edge=0.35, noise=0.02, pnoise=0.05, constant_left=False):
    """The GPU tests' input: a normalised guide = smooth colour image + a step edge at column W // 2 + noise, and p [B, n, H, W] correlated
    with its luminance plus noise, inside +-8 px.  constant_left: the guide is exactly constant left of column W // 3."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0.0, 1.0, H).view(1, 1, H, 1)
    xx = torch.linspace(0.0, 1.0, W).view(1, 1, 1, W)
    phase = torch.rand(B, 3, 1, 1, generator=g) * 6.28
    rgb = 0.45 + 0.2 * torch.sin(3.0 * xx + 2.0 * yy + phase) + edge * (xx > 0.5).float() * torch.tensor([0.6, 1.0, 0.4]).view(1, 3, 1, 1)
    rgb = (rgb + noise * torch.randn(B, 3, H, W, generator=g)).clamp(0.0, 1.0)
    if constant_left:
        rgb[..., :W // 3] = 0.5
    guide = torch.stack([(rgb[:, c] - MEAN[c]) / STD[c] for c in range(3)], dim=1).float()
    if constant_left:                                            # exactly constant after the fp32 normalisation too
        guide[..., :W // 3] = guide[..., :1, :1].expand(B, 3, H, W // 3)
    I = luminance(guide, torch.float32).unsqueeze(1)
    gain = torch.rand(B, n, 1, 1, generator=g) * 8.0 + 4.0
    p = (gain * (I - 0.6) + pnoise * torch.randn(B, n, H, W, generator=g)).clamp(-8.0, 8.0)
    return p.float(), guide


# ---- the cases of tests/test_gpu_postprocess.py, shared with tools/postprocess_bench.py (which records each case's kernel error and bar)
DEV = 'cuda'
EPS, SIGMA_COLOR = 1e-3, 0.1
ULP200 = 2.0 ** -16                                              # the spacing of fp32 in [128, 256)

# (B, n, H, W, r, batch stride in units of n H W)
SHARED = [(1, 1, 5, 7, 4, 1),                                    # the image is smaller than the window in both axes
          (2, 2, 33, 47, 1, 1),                                  # odd sizes, two heads, two samples, the smallest radius; H % 8 == 1
          (1, 1, 70, 131, 8, 1),                                 # several bands (guided) / tiles in both axes (bilateral), W % 4 != 0
          (2, 2, 33, 47, 1, 2)]                                  # pred is a slice of a tensor twice as wide: batch stride > n H W
GUIDED = SHARED + [(1, 3, 16, 300, 32, 1),                       # the largest radius, H < window < W, two strips of 192 columns
                   (1, 1, 20, 500, 8, 1),                        # three strips of 240 columns at the default radius
                   (1, 1, 17, 40, 5, 1)]                         # a one-row last band under a small radius: rows that leave the window late
BILATERAL = SHARED + [(1, 1, 40, 40, 16, 1)]                     # the largest radius


def case_id(case):
    return 'x'.join(str(v) for v in case[:4]) + '-r%d' % case[4] + ('-strided' if case[5] > 1 else '')


def sigma_space(r):
    return max(1.0, r / 2.0)


_cache = {}


def case(kind, case_):
    """(p, guide, q64, bar) of a case, computed once: bar = 2 x (max error of the fp32 variant against fp64 on this input) + 1e-6."""
    key = (kind,) + tuple(case_[:5])
    if key not in _cache:
        B, n, H, W, r = case_[:5]
        p, guide = scene(B, n, H, W, seed=1000 * B + 7 * H + W + r)
        if kind == 'guided':
            q64, q32 = guided_filter(p, guide, r, EPS), guided_filter_fp32(p, guide, r, EPS)
        else:
            q64 = joint_bilateral_filter(p, guide, r, sigma_space(r), SIGMA_COLOR)
            q32 = joint_bilateral_filter_fp32(p, guide, r, sigma_space(r), SIGMA_COLOR)
        _cache[key] = (p, guide, q64, 2.0 * float((q32.double() - q64).abs().max()) + 1e-6)
    return _cache[key]


def on_device(p, stride_units):
    """p on the device, contiguous or as the first half of the heads of a tensor twice as wide."""
    if stride_units == 1:
        return p.to(DEV)
    wide = torch.full((p.shape[0], p.shape[1] * stride_units) + tuple(p.shape[2:]), float('nan'), device=DEV)
    wide[:, :p.shape[1]] = p.to(DEV)
    view = wide[:, :p.shape[1]]
    assert not view.is_contiguous() and view.stride(0) == stride_units * p[0].numel()
    return view


def run_filter(kind, p_dev, guide_dev, r):
    """The operator under test on device tensors, with the cases' parameters."""
    from dualpixelface_amd import ops
    if kind == 'guided':
        return ops.guided_filter(p_dev, guide_dev, r, EPS)
    return ops.joint_bilateral_filter(p_dev, guide_dev, r, sigma_space(r), SIGMA_COLOR)
