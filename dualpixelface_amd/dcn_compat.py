"""Drop-in for the reference's pybind module ``DCN`` (src/module/dcn3d/src/vision.cpp:4-7).

    import dualpixelface_amd.dcn_compat as DCN        # or: sys.modules['DCN'] = dualpixelface_amd.dcn_compat
    out = DCN.deform_conv_forward(input, weight, bias, offset, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw,
                                  group, deformable_group, im2col_step)
    grad_input, grad_offset, grad_weight, grad_bias = DCN.deform_conv_backward(input, weight, bias, offset, grad_output, ...same ints...)

Same argument order, tensor layouts and error behaviour as deform_conv.h:10-29,49-69 / deform_conv_cuda.cu:18-285
(contiguous CUDA tensors required -> RuntimeError otherwise; results freshly allocated; runs on the current stream), so
the reference's own ``DeformConvFunction`` (functions/deform_conv_func.py:16-59) can call it unchanged.

``group`` and ``deformable_group`` go straight to the C ABI (weight ``[K, C / group, kd, kh, kw]``, offset
``[B, deformable_group * 3 T, Do, Ho, Wo]``): one native launch sequence for every grouping, no slicing, no copies and no
allocation beyond the results.  Group counts that do not divide the channel counts raise RuntimeError before anything runs.
That sequence is a gather tier (global loads per sample, global atomics for grad_input): at B=1, C=K=64, 4x64x96 it measured 3.4-4.9x
slower forward and 8-10.6x slower backward than the per-piece decomposition this module used before, whose pieces ran on the fast
single-group tiers (profiles/grouped_dcn_timings.txt).  Non-finite values: conv groups narrower than 32 channels share a matrix tile of
the block-diagonal weight, so a NaN or Inf in one conv group's samples or grad_output becomes NaN in the other groups of that tile.
"""
from . import ops
from ._lib import DpfError


def _check(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError('input must be a CUDA tensor')          # AT_ASSERTM at deform_conv_cuda.cu:44-47
        if not t.is_contiguous():
            raise RuntimeError('input tensor has to be contiguous')    # deform_conv_cuda.cu:41-42


def _check_groups(C, K, group, deformable_group):
    """deform_conv_cuda.cu:65-66: both kinds of group must divide the channel counts (the C ABI would answer DPF_ERR_INVALID_ARG)."""
    if C % group or K % group or C % deformable_group:
        raise RuntimeError('channels(%d) and channels_out(%d) must divide group(%d) / deformable_group(%d)' % (C, K, group, deformable_group))


def deform_conv_forward(input, weight, bias, offset, kernel_d, kernel_h, kernel_w, stride_d, stride_h, stride_w, pad_d, pad_h, pad_w,
                        dilation_d, dilation_h, dilation_w, group, deformable_group, im2col_step):
    _check(input, weight, bias, offset)
    if tuple(weight.shape[2:]) != (kernel_d, kernel_h, kernel_w):
        raise RuntimeError('Input shape and kernel shape wont match')   # deform_conv_cuda.cu:72-73
    if input.shape[1] != weight.shape[1] * group:
        raise RuntimeError('Input shape and kernel channels wont match')   # deform_conv_cuda.cu:75-76
    geo = ((stride_d, stride_h, stride_w), (pad_d, pad_h, pad_w), (dilation_d, dilation_h, dilation_w))
    x, w, b, off = input.float(), weight.float(), bias.float(), offset.float()
    _check_groups(x.shape[1], w.shape[0], group, deformable_group)
    try:
        return ops.deform_conv_forward_raw(x, w, b, off, *geo, group, deformable_group, im2col_step)
    except DpfError as e:
        raise RuntimeError(str(e))


def deform_conv_backward(input, weight, bias, offset, grad_output, kernel_d, kernel_h, kernel_w, stride_d, stride_h, stride_w, pad_d,
                         pad_h, pad_w, dilation_d, dilation_h, dilation_w, group, deformable_group, im2col_step):
    _check(input, weight, bias, offset)
    geo = ((stride_d, stride_h, stride_w), (pad_d, pad_h, pad_w), (dilation_d, dilation_h, dilation_w))
    x, w, b, off, go = input.float(), weight.float(), bias.float(), offset.float(), grad_output.float().contiguous()
    _check_groups(x.shape[1], w.shape[0], group, deformable_group)
    try:
        return list(ops.deform_conv_backward_raw(x, w, b, off, go, *geo, group, deformable_group, im2col_step))
    except DpfError as e:
        raise RuntimeError(str(e))
