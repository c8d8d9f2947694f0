"""Drop-in for the reference's pybind module ``deform_conv_cuda`` (src/module/dcn/src/deform_conv_cuda.cpp:687-697), the 2-D deformable
convolution behind DeformConv / DeformConvPack / ModulatedDeformConv / ModulatedDeformConvPack (src/module/dcn/deform_conv.py).

    import sys, dualpixelface_amd.dcn2d_compat
    sys.modules['deform_conv_cuda'] = dualpixelface_amd.dcn2d_compat      # before the reference's deform_conv.py is imported

The five functions take the reference's arguments in the reference's order (note kW before kH in the plain three) and fill the tensors
the caller passes, as the reference's autograd functions expect (deform_conv.py:39-46,62-77,114-119,128-137):

  * ``output``, ``gradOffset`` / ``grad_offset`` and ``grad_mask`` are overwritten;
  * ``gradInput`` / ``grad_input``, ``gradWeight`` / ``grad_weight`` and ``grad_bias`` are ADDED INTO -- the reference accumulates into the
    zero tensors its autograd functions pass (deform_conv_cuda.cpp:462-466,659-669);
  * ``scale`` multiplies the weight gradient (deform_conv_cuda.cpp:465);
  * the ``columns`` and ``ones`` buffers are accepted and ignored (the native kernels build no column matrix);
  * ``im2col_step`` must divide the batch (deform_conv.py:40), otherwise RuntimeError; it has no other effect.

CPU or non-contiguous tensors, a window that does not match the weight, channel counts that do not match and group counts that do not divide
the channels raise RuntimeError before anything runs.  Everything runs on the current stream through the C ABI
(dpf_deform_conv2d_forward / dpf_deform_conv2d_backward, include/dpf_hip.h): whole C, K <= 256, kh kw <= 49.
"""
import torch

from . import ops
from ._lib import DpfError


def _check(*ts):
    for t in ts:
        if not t.is_contiguous():
            raise RuntimeError('input tensor has to be contiguous')    # deform_conv_cuda.cpp:74,498-499
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError('input must be a CUDA tensor')
        if t.dtype != torch.float32:
            raise RuntimeError('input must be a float32 tensor, got %s' % t.dtype)


def _geometry(input, weight, offset, mask, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group):
    """shape_check (deform_conv_cuda.cpp:65-154) and its modulated counterpart (:507-515) -> (stride, pad, dil, output shape)."""
    if weight.dim() != 4 or input.dim() != 4:
        raise RuntimeError('4D input and 4D weight tensor expected but got: %s, %s' % (tuple(input.shape), tuple(weight.shape)))
    if kW <= 0 or kH <= 0 or dW <= 0 or dH <= 0 or dilationW <= 0 or dilationH <= 0:
        raise RuntimeError('kernel size, stride and dilation should be greater than zero')
    if (weight.shape[2], weight.shape[3]) != (kH, kW):
        raise RuntimeError('Input shape and kernel shape wont match: (%d x %d vs %d x %d).' % (kH, kW, weight.shape[2], weight.shape[3]))
    C, K = input.shape[1], weight.shape[0]
    if group < 1 or deformable_group < 1 or C % group or K % group or C % deformable_group:
        raise RuntimeError('channels(%d) and channels_out(%d) must divide group(%d) / deformable_group(%d)' % (C, K, group, deformable_group))
    if C != weight.shape[1] * group:
        raise RuntimeError('Input shape and kernel channels wont match: (%d vs %d).' % (C, weight.shape[1] * group))
    ho = (input.shape[2] + 2 * padH - (dilationH * (kH - 1) + 1)) // dH + 1
    wo = (input.shape[3] + 2 * padW - (dilationW * (kW - 1) + 1)) // dW + 1
    if ho <= 0 or wo <= 0:
        raise RuntimeError('Given input size: (%d x %d x %d). Calculated output size: (%d x %d x %d). Output size is too small'
                           % (C, input.shape[2], input.shape[3], K, ho, wo))
    B, T = input.shape[0], kH * kW
    if tuple(offset.shape) != (B, deformable_group * 2 * T, ho, wo):
        raise RuntimeError('invalid offset shape %s, expected %s' % (tuple(offset.shape), (B, deformable_group * 2 * T, ho, wo)))
    if mask is not None and tuple(mask.shape) != (B, deformable_group * T, ho, wo):
        raise RuntimeError('invalid mask shape %s, expected %s' % (tuple(mask.shape), (B, deformable_group * T, ho, wo)))
    return (dH, dW), (padH, padW), (dilationH, dilationW), (B, K, ho, wo)


def _expect(t, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError('invalid %s shape %s, expected %s' % (name, tuple(t.shape), tuple(shape)))


def _step(im2col_step, batch):
    if im2col_step < 1 or batch % im2col_step:
        raise RuntimeError('im2col step must divide batchsize')        # deform_conv.py:40, deform_conv_cuda.cpp:185


def _run(fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except DpfError as e:
        raise RuntimeError(str(e))


def deform_conv_forward_cuda(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group,
                             deformable_group, im2col_step):
    _check(input, weight, offset, output)
    s, p, d, oshape = _geometry(input, weight, offset, None, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    _step(im2col_step, input.shape[0])
    _expect(output, oshape, 'output')
    _run(ops.deform_conv2d_forward_raw, input, weight, None, offset, None, s, p, d, group, deformable_group, out=output)
    return 1


def deform_conv_backward_input_cuda(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, kH, dW, dH, padW, padH,
                                    dilationW, dilationH, group, deformable_group, im2col_step):
    _check(input, offset, gradOutput, gradInput, gradOffset, weight)
    s, p, d, oshape = _geometry(input, weight, offset, None, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    _step(im2col_step, input.shape[0])
    _expect(gradOutput, oshape, 'gradOutput')
    _expect(gradInput, input.shape, 'gradInput')
    _expect(gradOffset, offset.shape, 'gradOffset')
    gi = _run(ops.deform_conv2d_backward_raw, input, weight, None, offset, None, gradOutput, s, p, d, group, deformable_group,
              want=(True, True, False, False, False), goff_out=gradOffset)[0]
    gradInput.add_(gi)
    return 1


def deform_conv_backward_parameters_cuda(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW, dH, padW, padH, dilationW,
                                         dilationH, group, deformable_group, scale, im2col_step):
    _check(input, offset, gradOutput, gradWeight)
    s, p, d, oshape = _geometry(input, gradWeight, offset, None, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    _step(im2col_step, input.shape[0])
    _expect(gradOutput, oshape, 'gradOutput')
    # The reference does not pass the weight here, so gradWeight stands in for it: deform_conv2d_backward_raw takes [K, C / group, kh, kw]
    # from its shape, and with only grad_weight wanted the C entry launches neither the repack nor the data kernel -- the weight operand's
    # VALUES are never read on this path (dpf_deform_conv2d_backward, include/dpf_hip.h RESULTS).
    gw = _run(ops.deform_conv2d_backward_raw, input, gradWeight, None, offset, None, gradOutput, s, p, d, group, deformable_group,
              want=(False, False, False, True, False))[3]
    gradWeight.add_(gw, alpha=float(scale))
    return 1


def modulated_deform_conv_cuda_forward(input, weight, bias, ones, offset, mask, output, columns, kernel_h, kernel_w, stride_h, stride_w,
                                       pad_h, pad_w, dilation_h, dilation_w, group, deformable_group, with_bias):
    _check(input, weight, offset, mask, output)
    if with_bias:
        _check(bias)
    s, p, d, oshape = _geometry(input, weight, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                                group, deformable_group)
    _expect(output, oshape, 'output')
    if with_bias:
        _expect(bias, (weight.shape[0],), 'bias')
    _run(ops.deform_conv2d_forward_raw, input, weight, bias if with_bias else None, offset, mask, s, p, d, group, deformable_group, out=output)


def modulated_deform_conv_cuda_backward(input, weight, bias, ones, offset, mask, columns, grad_input, grad_weight, grad_bias, grad_offset,
                                        grad_mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                        dilation_w, group, deformable_group, with_bias):
    _check(input, weight, offset, mask, grad_input, grad_weight, grad_offset, grad_mask, grad_output)
    if with_bias:
        _check(bias, grad_bias)
    s, p, d, oshape = _geometry(input, weight, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                                group, deformable_group)
    _expect(grad_output, oshape, 'grad_output')
    _expect(grad_input, input.shape, 'grad_input')
    _expect(grad_weight, weight.shape, 'grad_weight')
    _expect(grad_offset, offset.shape, 'grad_offset')
    _expect(grad_mask, mask.shape, 'grad_mask')
    if with_bias:
        _expect(bias, (weight.shape[0],), 'bias')
        _expect(grad_bias, bias.shape, 'grad_bias')
    gi, _, _, gw, gb = _run(ops.deform_conv2d_backward_raw, input, weight, bias if with_bias else None, offset, mask, grad_output, s, p, d,
                            group, deformable_group, want=(True, True, True, True, bool(with_bias)), goff_out=grad_offset, gm_out=grad_mask)
    grad_input.add_(gi)
    grad_weight.add_(gw)
    if with_bias:
        grad_bias.add_(gb)
