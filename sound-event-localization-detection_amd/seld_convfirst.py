"""Autograd wrapper of the first encoder block with its convolution recomputed in place (csrc/convfirst.hip):
Conv3x3(4 -> 64) -> BatchNorm2d -> ReLU -> MaxPool2d((1, 2)) of model_crnn.py:5-17 as three launches forward (statistics,
finalise, apply) and four backward (reduction, finalise, weight gradient, fixed-order sum).  The 65.5 MB convolution output and its equally
large gradient are never written: only the 4 MB input and the BatchNorm coefficients are kept for the backward pass.
Everything runs on the caller's stream."""
import torch
import torch.nn as nn

import seld_convtail
import seld_native

enabled = True        # flipped by the trainer from Config.FUSED_FIRST_BLOCK


def applicable(block, x):
    """``block``: a ConvBlock; ``x``: its input.  The training configuration of the shared encoder's first block only:
    everything else (fp32, eval, other channel counts, an input that needs a gradient) keeps the general path."""
    if not (enabled and seld_convtail.enabled and x.is_cuda and x.dim() == 4 and torch.is_grad_enabled()
            and not x.requires_grad):
        return False
    import model_crnn
    conv, bn, pool = block.conv, block.bn, block.pool
    if not (model_crnn._Conv3x3.enabled and type(conv) is nn.Conv2d and conv.kernel_size == (3, 3)
            and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros" and conv.weight.requires_grad):
        return False
    if not (type(bn) is nn.BatchNorm2d and bn.training and bn.affine and bn.track_running_stats
            and bn.momentum is not None and bn.weight.dtype == torch.float32 and bn.weight.requires_grad
            and bn.bias.requires_grad):
        return False
    if type(pool) is not nn.MaxPool2d:
        return False
    k = pool.kernel_size if isinstance(pool.kernel_size, tuple) else (pool.kernel_size,) * 2
    s = pool.stride if isinstance(pool.stride, tuple) else (pool.stride,) * 2
    if tuple(k) != (1, 2) or tuple(s) != (1, 2) or pool.padding not in (0, (0, 0)) or pool.ceil_mode \
            or pool.dilation not in (1, (1, 1)):
        return False
    # bf16 compute: a bf16 input (run_cnn_blocks casts under autocast) or bf16 autocast over an fp32 one is the
    # caller's business -- only an input that already IS bf16 channels-last is taken
    return seld_native.convfirst_applicable(x, conv.weight)


class _ConvFirst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, conv_weight, bn_weight, bn_bias, running_mean, running_var, momentum, eps):
        y, mean_invstd, scale_shift = seld_native.convfirst_forward(x, conv_weight, bn_weight, bn_bias, running_mean,
                                                                    running_var, momentum, eps)
        # the bf16 values the kernels multiplied with: the working copy itself, or autocast's rounding of the fp32 weight
        ctx.save_for_backward(x, conv_weight, mean_invstd, scale_shift)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, conv_weight, mean_invstd, scale_shift = ctx.saved_tensors
        dw = torch.empty_like(conv_weight)                # the parameter's own layout and dtype: no cast, no copy
        dw, dgamma, dbeta = seld_native.convfirst_backward(x, conv_weight, dy, mean_invstd, scale_shift, dw)
        return None, dw, dgamma, dbeta, None, None, None, None


def first_block(block, x):
    bn = block.bn
    if seld_convtail._collected is not None:
        seld_convtail._collected.append(bn.num_batches_tracked)
    else:
        bn.num_batches_tracked.add_(1)
    return _ConvFirst.apply(x, block.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum,
                            bn.eps)
