"""Client-grouped layers for the batched 2-D image engine on the hand-written kernels (``conv2d_fd.hip``,
``conv2d_ws.hip``, ``conv2d_thin.hip``, ``conv2d_any.hip``, ``conv2d_wg.hip``, ``linear_g.hip``, ``gn_pool.hip``).

The small models of the reference's entry points (``lenet5``, ``cnn_cifar10/100``, the EMNIST CNNs, ``vgg11/16`` —
``fedml_experiments/standalone/subavg/main_subavg.py:143-158``) run G clients of a lockstep step as one pass over
group-stacked tensors ``[G*B, C, H, W]``: a deep copy of the model whose ``Conv2d`` / ``Linear`` / ``GroupNorm`` /
``MaxPool2d(2, 2)`` modules are replaced by grouped twins reading the clients' parameter rows (``[G, *shape]`` views of theta):

* ``Conv2d`` (stride 1, any kernel size and channel count) -> :class:`HipConv2dFn`: forward and stride-1 data
  gradient on the LDS-staged MFMA kernel of ``conv2d_fd.hip`` where the contraction channel count is a multiple of 8
  and at least 64 (``conv2d_fd_ok``; both directions read the forward weight image: no transposed image is packed
  for such a layer), on the implicit-GEMM MFMA kernel of ``conv2d_any.hip`` otherwise (narrow layers) and
  everywhere with ``NIDT_B2D_FD=0``; the thin first layers (at most 4 input channels, ``conv2d_thin_ok``) run their
  forward and their weight / bias gradient on ``conv2d_thin.hip`` (a dense contraction over k k Cin, the fp32
  weights read in place with no image packed, the gradient split over positions and summed in a fixed order;
  ``NIDT_B2D_THIN=0`` routes them as every other layer); the weight-bound deep 3 x 3 layers on small maps
  (``conv2d_ws_ok``: vgg's layers from 128 input channels up, 16 x 16 maps and smaller) run forward and data
  gradient on ``conv2d_ws.hip``, which reads the clients' fp32 blocks in place, so that such a layer packs no image at
  all, in training and in evaluation (``NIDT_B2D_WS=0`` keeps the image paths, 2 routes every served layer);
  weight and bias gradient of the other layers on the MFMA
  kernel of ``conv2d_wg.hip``, which owns each output element and writes fp32 in the parameter layout, the bf16 weight images
  from one ``conv2d_pack_w`` launch; ``NIDT_B2D_WGRAD=0`` keeps the staged fp32 weight-gradient kernel of
  ``conv2d_any.hip`` with its framework partial sum, bias sum and packing; the activations stay channels-last
  (``torch.channels_last`` views), bf16;
* ``Linear`` -> :class:`HipLinearFn`: forward, data gradient and weight / bias gradient on the MFMA kernels of
  ``linear_g.hip``, which read the fp32 weight rows in place (rounded to bf16 in registers, no bf16 weight copy) and
  write fp32-accumulated fp32 weight gradients in a fixed order; ``NIDT_B2D_LINEAR=0`` (and the CPU) keeps one
  batched library GEMM per layer (``baddbmm`` over the client axis);
* ``GroupNorm`` and, inside an ``nn.Sequential``, the ``ReLU`` and the ``MaxPool2d(2, 2)`` that follow it ->
  :class:`HipGroupNormFn`: one forward and one backward kernel of ``gn_pool.hip`` over the channels-last bf16
  activation, the per-client affine read from the parameter rows in place, the ReLU mask and the pooling argmax
  recomputed in the backward (no mask or index tensor); the absorbed modules become ``nn.Identity`` at their
  indices.  A ``MaxPool2d(2, 2)`` on its own -> :class:`HipMaxPool2dFn` (same file).  ``NIDT_B2D_GN=0``, the CPU and
  the shapes outside ``gn2d_ok`` / ``pool2d_ok`` run the framework expression (``group_norm`` without affine, the
  per-client affine, ``relu``, ``max_pool2d``);
* everything else (other ReLUs, dropout, flatten, functional pooling) is per-sample and runs unchanged on the
  stacked batch.

The model's own ``forward`` runs as written, so the layer order and every view/flatten are the reference's.
"""
from __future__ import annotations

import copy
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


_stream = ops.stream


def _nhwc_bf16(x):
    """[N, C, H, W]-shaped tensor -> contiguous channels-last bf16 [N, H, W, C] (no copy for a channels-last bf16
    input)."""
    t = x.permute(0, 2, 3, 1)
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t if t.is_contiguous() else t.contiguous()


def pack_conv_w(w):
    """fp32 [G, Cout, Cin, k, k] -> bf16 forward image [G, ceil64(Cout), k*k, ceil8(Cin)] (zero padded)."""
    G, co, ci, k, _ = w.shape
    img = w.permute(0, 1, 3, 4, 2).reshape(G, co, k * k, ci)
    img = F.pad(img, (0, (-ci) % 8, 0, 0, 0, (-co) % 64))
    return img.to(torch.bfloat16).contiguous()


def pack_conv_wt(w):
    """fp32 [G, Cout, Cin, k, k] -> the data-gradient image [G, ceil64(Cin), k*k, ceil8(Cout)]: the flipped kernel
    with input and output channels exchanged (dX = conv(dY, W^T flipped), padding k - 1 - p)."""
    G, co, ci, k, _ = w.shape
    img = w.flip(3, 4).permute(0, 2, 3, 4, 1).reshape(G, ci, k * k, co)
    img = F.pad(img, (0, (-co) % 8, 0, 0, 0, (-ci) % 64))
    return img.to(torch.bfloat16).contiguous()


def _hip_wgrad_on():
    return os.environ.get("NIDT_B2D_WGRAD", "1") != "0"


WG_MIN_BLOCKS = 64


def conv2d_wg_lds_bytes(k, Wo, cin):
    """The dynamic LDS of a ``conv2d_wg`` launch: the launcher's own arithmetic (two buffers of a 32 x 72 dY tile and
    of ``nu`` union rows of ci tile + 8 bf16 elements, nu = 32 + (k - 1) min(32, 1 + ceil(31 / Wo)))."""
    nu = 32 + (k - 1) * min(32, 1 + (31 + Wo - 1) // Wo)
    return 2 * 2 * (32 * 72 + nu * ((16 if cin <= 16 else 64) + 8))


def conv2d_wg_ok(k, Wo, G, cin, cout):
    """The layers whose weight gradient runs on ``conv2d_wg``; everything else keeps ``conv2d_any_wgrad``.

    * the launcher's rule: kernels up to 7 x 7 whose LDS tiles fit 64 KiB (of those only a 7 x 7 kernel with more
      than 16 input channels on a 1-wide output map does not: 73 728 B);
    * the measured rule (``profiles/r11_conv2d_wgrad.txt``): one block owns each output element and walks the whole
      contraction, so a launch of fewer than ``WG_MIN_BLOCKS`` blocks (clients x ci tiles x co tiles x k) is
      latency-bound.  At 8 clients x 64 images the 24- to 48-block launches ran at 0.49x - 0.99x of the parent path
      on five layers (1.13x - 1.40x on three others, which this rule gives up); the smallest launch measured above
      48 blocks had 192 (3.2x), and every launch of 192 blocks or more was 3.2x - 11x faster.  The threshold of 64 is
      interpolated between 48 (0.99x) and 192: no launch of 49 .. 191 blocks was measured.  The rule looks at the
      block count alone, not at the contraction length B Ho Wo, the other half of "latency-bound": among the 40-block
      launches 128 steps ran at 0.80x, 200 steps at 1.24x - 1.40x and 1568 steps at 0.86x and at 1.13x, so the
      measurements give no length threshold."""
    blocks = G * (1 if cin <= 16 else (cin + 63) // 64) * ((cout + 63) // 64) * k
    return k <= 7 and conv2d_wg_lds_bytes(k, Wo, cin) <= 65536 and blocks >= WG_MIN_BLOCKS


def _hip_fd_on():
    return os.environ.get("NIDT_B2D_FD", "1") != "0"


def conv2d_fd_lds_bytes(k, Wo):
    """The dynamic LDS of a ``conv2d_fd`` launch that writes a ``Wo``-wide map: the launcher's own arithmetic (two
    64 x 72 bf16 weight tiles and ``nu`` union rows of 72, nu = 64 + (k - 1) min(64, 1 + ceil(63 / Wo)))."""
    nu = 64 + (k - 1) * min(64, 1 + (63 + Wo - 1) // Wo)
    return 2 * 72 * (2 * 64 + nu)


FD_MIN_C = 64


def conv2d_fd_served(k, pad, W, cin, cout, dgrad):
    """The launcher's rule for a layer described by its forward (input width ``W``): kernels up to 7 x 7, the
    contraction channel count (cin forward, cout data gradient; its stride is the same number here) a multiple of 8,
    padding within the kernel for the data gradient, LDS within 64 KiB for the width of the map written."""
    Wo = W if dgrad else W + 2 * pad - k + 1
    return (1 <= k <= 7 and (cout if dgrad else cin) % 8 == 0 and pad >= 0 and (pad <= k - 1 or not dgrad)
            and Wo > 0 and conv2d_fd_lds_bytes(k, Wo) <= 65536)


def conv2d_fd_ok(k, pad, W, cin, cout, dgrad):
    """The layers whose forward / data gradient runs on ``conv2d_fd``; everything else keeps ``conv2d_any_fwd``.

    * the launcher's rule (``conv2d_fd_served``);
    * the measured rule (``profiles/r13_conv2d_fd.txt``): at least ``FD_MIN_C`` contraction channels.  A step of the
      kernel is one tap of one 64-channel chunk, in 32-deep MFMAs, behind a barrier; with 16 channels every MFMA is
      half padding and a 5 x 5 kernel takes 25 such steps where the old kernel walks the 400-long contraction in 13
      unsynchronised ones: LeNet5_cifar's 6 -> 16 data gradient ran at 0.45x / 0.42x of the old kernel (100 x 16 /
      8 x 64).  With 32 channels (the EMNIST CNNs' 32 -> 64 forward) a step issues half its MFMAs per barrier:
      0.88x / 0.85x at k = 5, 1.00x / 0.98x at k = 3.  Every launch measured with 64 or more contraction channels
      was faster, 1.58x - 2.96x forward and 1.81x - 2.98x for the data gradient with its pack, against a run-to-run
      spread of 1 - 3 percent.  Nothing was measured at 40 .. 56 channels; they stay on the old kernel."""
    return conv2d_fd_served(k, pad, W, cin, cout, dgrad) and (cout if dgrad else cin) >= FD_MIN_C


def _ws_mode():
    """``NIDT_B2D_WS``: 0 = no layer on ``conv2d_ws``, 1 = the layers ``conv2d_ws_ok`` accepts, 2 = every layer the
    launcher serves (tests and measurements).  The default is 1: the vgg11 train step took 0.73 and its evaluation
    0.40 of the time with 0 at 100 clients x 16 images, 0.96 and 0.77 at 8 x 64, against a [min .. max] spread of the
    path with 0 below 1 percent (``profiles/r16_conv2d_ws.txt``)."""
    return int(os.environ.get("NIDT_B2D_WS", "1"))


WS_MAX_ROWS = 768
WS_MIN_CIN = 128


def conv2d_ws_tile(k, pad, B, H, W, dgrad):
    """(positions per block, slab rows, dynamic LDS bytes) of a ``conv2d_ws`` launch, or None where the slab of whole
    padded samples does not fit: the launcher's own arithmetic.  A tile of ``tm`` positions touches at most ``ns``
    samples of P = Ho Wo positions of the map written (tm / P if P divides tm, 1 if tm divides P,
    floor((tm + 2 P - 2) / P) otherwise, B at most), each a slab of (Ho + k - 1)(Wo + k - 1) rows of 48 bytes, next to
    k k weight tiles of 3088 bytes; at most ``WS_MAX_ROWS`` rows and 64 KiB; 256 positions from B P = 256 up where
    they fit, else 64."""
    Ho, Wo = (H, W) if dgrad else (H + 2 * pad - k + 1, W + 2 * pad - k + 1)
    if Ho <= 0 or Wo <= 0:
        return None
    P = Ho * Wo

    def tile(tm):
        ns = tm // P if tm % P == 0 else 1 if P % tm == 0 else (tm + 2 * P - 2) // P
        rows = min(ns, B) * (Ho + k - 1) * (Wo + k - 1)
        lds = 2 * (k * k * (64 * 24 + 8) + rows * 24)
        return (tm, rows, lds) if rows <= WS_MAX_ROWS and lds <= 65536 else None

    small = tile(64)
    return small and ((B * P >= 256 and tile(256)) or small)


def conv2d_ws_served(k, pad, B, H, W, cin, cout, dgrad):
    """The launcher's rule of ``conv2d_ws`` for a layer described by its forward (``B`` images of ``H`` x ``W`` per
    client): kernels up to 3 x 3, the contraction channel count (cin forward, cout data gradient; its stride is the
    same number here) a multiple of 8, padding within the kernel for the data gradient, and the whole padded samples
    of a tile within the LDS budget (``conv2d_ws_tile``): small maps."""
    return (1 <= k <= 3 and (cout if dgrad else cin) % 8 == 0 and pad >= 0 and (pad <= k - 1 or not dgrad)
            and conv2d_ws_tile(k, pad, B, H, W, dgrad) is not None)


def conv2d_ws_ok(k, pad, B, H, W, cin, cout, dgrad):
    """The layers whose forward / data gradient runs on ``conv2d_ws``; everything else keeps its image and ``conv2d_fd`` /
    ``conv2d_any_fwd``.

    * the launcher's rule (``conv2d_ws_served``) for this direction AND for the forward: the data gradient goes to
      ``conv2d_ws`` only together with the forward, so that the layer packs nothing.  With the forward on ``conv2d_ws``
      the ``conv2d_pack_w`` launch serves ``conv2d_fd``'s data gradient alone and belongs to its cost;
    * the measured rule (``profiles/r16_conv2d_ws.txt``, the 3 x 3, pad 1 layers of vgg11 / vgg16 on 16 x 16 .. 2 x 2
      maps, 100 clients x 16 images / 8 x 64, the parent path interleaved in the same run): k = 3 and at least
      ``WS_MIN_CIN`` = 128 input channels.  Forward against ``conv2d_pack_w`` + ``conv2d_fd``: 1.28x - 4.39x / 1.23x -
      1.70x on the six layers from 128 channels up, each beyond the parent's [min .. max]; 64 -> 128 on 16 x 16 maps
      ran 1.13x / 1.14x with a difference equal to the parent's spread (0.019 / 0.006 ms), not beyond it: it stays.
      ``HipConv2dFn`` forward + backward, nothing packed against the parent routing: 1.11x - 1.92x at 100 x 16, all
      six beyond the spread; at 8 x 64 three are beyond it (128 -> 128, 256 -> 256, 512 -> 512 on 4 x 4: 1.06x -
      1.19x) and three are inside it (1.00x - 1.05x), none slower.  Kernel against kernel the data gradient alone
      is NOT always faster (0.52x on 2 x 2 maps at 100 x 16, 0.65x - 0.92x on 4 of 7 layers at 8 x 64: it re-reads
      fp32 where ``conv2d_fd`` reads a bf16 image that the forward paid for); what it saves is the pack (0.71 ms
      against 0.11 ms of lost kernel time on that 2 x 2 layer).  The column "``conv2d_fd`` data gradient + pack" was
      not timed as one call: it is the sum of two columns; the ``HipConv2dFn`` column is the direct measurement.
      Not measured: k = 1 and 2, paddings other than 1, non-square maps, channel counts off the vgg tables, and a
      layer with the forward on ``conv2d_ws`` and the data gradient on ``conv2d_fd``; k = 1, 2 stay on the parent
      path, the others follow the rule above."""
    return (conv2d_ws_served(k, pad, B, H, W, cin, cout, dgrad) and conv2d_ws_served(k, pad, B, H, W, cin, cout, False)
            and k == 3 and cin >= WS_MIN_CIN)


def _hip_thin_on():
    return os.environ.get("NIDT_B2D_THIN", "1") != "0"


def conv2d_thin_kp(k, cin):
    """The padded dense contraction of ``conv2d_thin.hip``: k k cin rounded up to 32."""
    return (k * k * cin + 31) // 32 * 32


def conv2d_thin_served(k, cin):
    """The launcher's rule of ``conv2d_thin_fwd`` / ``conv2d_thin_wgrad``: at most 4 input channels, kernels up to
    7 x 7, a padded contraction of at most 96 (k = 7 only with one channel, k = 5 with up to three)."""
    return 1 <= k <= 7 and 1 <= cin <= 4 and conv2d_thin_kp(k, cin) <= 96


def conv2d_thin_ok(k, cin, cout):
    """The layers whose forward and weight / bias gradient run on ``conv2d_thin.hip`` (the first layers, Cin = 1 or
    3): the launcher's rule (``conv2d_thin_served``) alone.  The measurements add no rule
    (``profiles/r15_conv2d_thin.txt``): the six first layers of the zoo and of the EMNIST CNNs (1->20, 3->6, 3->64,
    1->32 at k = 5, 3->64 and 1->32 at k = 3) all beat the parent's routed paths at 100 clients x 16 images and at
    8 x 64, by far more than the 1 - 4 percent [min .. max] spread of those paths: the forward 1.28x - 2.49x and
    1.18x - 2.26x against ``conv2d_pack_w`` + ``conv2d_any_fwd``, the weight + bias gradient 2.93x - 4.85x against
    ``conv2d_wg`` and 14.9x - 35x against the staged fp32 kernel that ``WG_MIN_BLOCKS`` routes to at 8 x 64.  Other
    Cout, kernel sizes 1, 2, 4, 6, 7 and Cin = 2, 4 were not timed."""
    return conv2d_thin_served(k, cin)


def conv2d_thin_scratch(G, B, Ho, Wo, cout, k, cin, device, splits=0):
    """The fp32 scratch of a ``conv2d_thin_wgrad`` launch: one 64 x Kp dW partial and 64 dB partials per (client, co
    tile, position split), the number of splits from ``conv2d_thin_splits`` (a function of the shapes alone)."""
    S = ops.ext().conv2d_thin_splits(G, B, Ho, Wo, cout, splits)
    return torch.empty(G * ((cout + 63) // 64) * S * 64 * (conv2d_thin_kp(k, cin) + 1), device=device,
                       dtype=torch.float32)


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _client_blocks(w):
    """w [G, ...] as (tensor whose clients are contiguous blocks at one stride, that stride in elements)."""
    if not (w.dtype == torch.float32 and w[0].is_contiguous() and (w.shape[0] == 1 or w.stride(0) >= w[0].numel())):
        w = w.float().contiguous()
    return w, (w.stride(0) if w.shape[0] > 1 else w[0].numel())


def pack_conv_images(w, transposed):
    """``pack_conv_w(w)`` and, if asked for, ``pack_conv_wt(w)`` (else None) by one ``conv2d_pack_w`` launch that
    reads the clients' fp32 blocks where they lie."""
    G, co, ci, k, _ = w.shape
    w, ldw = _client_blocks(w)
    wp = torch.empty(G, (co + 63) // 64 * 64, k * k, (ci + 7) // 8 * 8, device=w.device, dtype=torch.bfloat16)
    wt = torch.empty(G, (ci + 63) // 64 * 64, k * k, (co + 7) // 8 * 8, device=w.device,
                     dtype=torch.bfloat16) if transposed else None
    ops.ext().conv2d_pack_w(w.data_ptr(), ldw, wp.data_ptr(), wt.data_ptr() if transposed else 0, G, co, ci, k,
                            _stream())
    return wp, wt


class HipConv2dFn(torch.autograd.Function):
    """Grouped stride-1 conv: x [G*B, Cin, H, W] (any strides), w [G, Cout, Cin, k, k] fp32, b [G, Cout] or None.
    With ``NIDT_B2D_WGRAD=1`` (the default) the weight images come from ``conv2d_pack_w`` and the weight / bias
    gradients from ``conv2d_wg`` (``conv2d_wg.hip``), in the parameter layout; 0 keeps the framework packing and
    ``conv2d_any_wgrad`` with its partial sums.  With ``NIDT_B2D_FD=1`` (the default) the forward and the data
    gradient of the layers ``conv2d_fd_ok`` accepts run on ``conv2d_fd`` (``conv2d_fd.hip``); the data gradient then
    reads the saved forward image and no transposed image is packed; 0 keeps ``conv2d_any_fwd`` for both.  With
    ``NIDT_B2D_THIN=1`` (the default) a layer that ``conv2d_thin_ok`` accepts runs its forward on ``conv2d_thin_fwd``
    (whatever the other two switches say: no image is packed) and, with ``NIDT_B2D_WGRAD=1``, its weight / bias
    gradient on ``conv2d_thin_wgrad``; its data gradient (tests only) stays on ``conv2d_any_fwd``.  With
    ``NIDT_B2D_WS=1`` (the default) each direction that ``conv2d_ws_ok`` accepts (2: that ``conv2d_ws_served`` accepts)
    runs on ``conv2d_ws`` on the fp32 blocks in place; ``conv2d_pack_w`` is launched only if some direction of the
    layer still reads an image."""

    @staticmethod
    def forward(ctx, x, w, b, G, pad):
        m = ops.ext()
        N, ci, H, W = x.shape
        co, k = w.shape[1], w.shape[3]
        assert N % G == 0 and w.shape[0] == G and w.shape[2] == ci
        B = N // G
        xs = _nhwc_bf16(x)
        Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
        y = torch.empty(N, Ho, Wo, co, device=x.device, dtype=torch.bfloat16)
        ctx.new = _hip_wgrad_on()
        ctx.thin = _hip_thin_on() and conv2d_thin_ok(k, ci, co)
        ctx.G, ctx.pad, ctx.has_b = G, pad, b is not None
        if ctx.thin:  # the fp32 weights and bias read where they lie: no image, no pack launch
            wb, ldw = _client_blocks(w.detach())
            bb, ldb = _client_blocks(b.detach()) if b is not None else (None, 0)
            m.conv2d_thin_fwd(xs.data_ptr(), wb.data_ptr(), ldw, bb.data_ptr() if b is not None else 0, ldb,
                              y.data_ptr(), G, B, H, W, ci, ci, co, k, pad, _stream())
            ctx.fd_d = ctx.ws_d = False  # a data gradient (tests only) packs its transposed image in the backward
            ctx.save_for_backward(xs, w, None)
            return y.permute(0, 3, 1, 2)
        fd, ws = _hip_fd_on(), _ws_mode()
        ws_rule = conv2d_ws_served if ws == 2 else conv2d_ws_ok
        ws_f = ws > 0 and ws_rule(k, pad, B, H, W, ci, co, False)
        ctx.ws_d = ws > 0 and ctx.needs_input_grad[0] and ws_rule(k, pad, B, H, W, ci, co, True)
        ctx.fd_d = fd and ctx.needs_input_grad[0] and not ctx.ws_d and conv2d_fd_ok(k, pad, W, ci, co, True)
        # the forward image: read by every forward kernel but conv2d_ws and by conv2d_fd's data gradient; the
        # transposed image: conv2d_any_fwd's data gradient.  A layer with both directions on conv2d_ws packs nothing
        need_img = not ws_f or ctx.fd_d
        need_t = ctx.needs_input_grad[0] and not (ctx.fd_d or ctx.ws_d)
        wp = wt = None
        if ctx.new and (need_img or need_t):
            wp, wt = pack_conv_images(w.detach(), need_t)
        elif need_img:
            wp = pack_conv_w(w.detach())
        bias = b.detach().float().contiguous() if b is not None and not ws_f else None
        if ws_f:  # the fp32 weights and bias read where they lie
            xs = _aligned16(xs)
            wb, ldw = _client_blocks(w.detach())
            bb, ldb = _client_blocks(b.detach()) if b is not None else (None, 0)
            m.conv2d_ws(xs.data_ptr(), wb.data_ptr(), ldw, bb.data_ptr() if b is not None else 0, ldb, y.data_ptr(),
                        G, B, H, W, ci, ci, co, k, pad, 0, _stream())
        elif fd and conv2d_fd_ok(k, pad, W, ci, co, False):
            xs = _aligned16(xs)
            m.conv2d_fd(xs.data_ptr(), wp.data_ptr(), bias.data_ptr() if bias is not None else 0, y.data_ptr(), G, B,
                        H, W, ci, ci, co, k, pad, 0, _stream())
        else:
            m.conv2d_any_fwd(xs.data_ptr(), wp.data_ptr(), bias.data_ptr() if bias is not None else 0, y.data_ptr(),
                             G, B, H, W, ci, ci, co, k, pad, _stream())
        ctx.save_for_backward(xs, w, wp if ctx.fd_d else wt)  # the data gradient on conv2d_fd reads the forward image
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        m = ops.ext()
        xs, w, wt = ctx.saved_tensors  # wt: the forward image when ctx.fd_d, else the transposed image or None
        G, pad = ctx.G, ctx.pad
        N, H, W, ci = xs.shape
        co, k = w.shape[1], w.shape[3]
        B = N // G
        dy = _nhwc_bf16(gy)
        Ho, Wo = dy.shape[1], dy.shape[2]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dxs = torch.empty(N, H, W, ci, device=xs.device, dtype=torch.bfloat16)
            if ctx.ws_d:
                dy = _aligned16(dy)
                wb, ldw = _client_blocks(w.detach())
                m.conv2d_ws(dy.data_ptr(), wb.data_ptr(), ldw, 0, 0, dxs.data_ptr(), G, B, H, W, ci, co, co, k, pad, 1,
                            _stream())
            elif ctx.fd_d:
                dy = _aligned16(dy)
                m.conv2d_fd(dy.data_ptr(), wt.data_ptr(), 0, dxs.data_ptr(), G, B, H, W, ci, co, co, k, pad, 1,
                            _stream())
            else:
                if wt is None:
                    wt = pack_conv_wt(w.detach())
                m.conv2d_any_fwd(dy.data_ptr(), wt.data_ptr(), 0, dxs.data_ptr(), G, B, Ho, Wo, co, co, ci, k,
                                 k - 1 - pad, _stream())
            dx = dxs.permute(0, 3, 1, 2)
        want_b = ctx.has_b and ctx.needs_input_grad[2]
        if ctx.new and ctx.thin:
            if ctx.needs_input_grad[1] or want_b:
                dw = torch.empty(G, co, ci, k, k, device=xs.device, dtype=torch.float32)
                if want_b:
                    db = torch.empty(G, co, device=xs.device, dtype=torch.float32)
                part = conv2d_thin_scratch(G, B, Ho, Wo, co, k, ci, xs.device)
                m.conv2d_thin_wgrad(xs.data_ptr(), dy.data_ptr(), dw.data_ptr(), co * ci * k * k,
                                    db.data_ptr() if want_b else 0, co, part.data_ptr(), part.numel(), 0, G, B, H, W,
                                    ci, ci, co, k, pad, _stream())
            return dx, dw, db, None, None
        if ctx.new and conv2d_wg_ok(k, Wo, G, ci, co):
            if ctx.needs_input_grad[1] or want_b:
                # dB comes from the dY tiles that the dW blocks stage: the kernel cannot skip dW, so a bias-only
                # gradient (no layer of the zoo asks for one) still computes and returns the whole dw
                dw = torch.empty(G, co, ci, k, k, device=xs.device, dtype=torch.float32)
                if want_b:
                    db = torch.empty(G, co, device=xs.device, dtype=torch.float32)
                m.conv2d_wg(xs.data_ptr(), dy.data_ptr(), dw.data_ptr(), co * ci * k * k,
                            db.data_ptr() if want_b else 0, co, G, B, H, W, ci, ci, co, k, pad, _stream())
            return dx, dw, db, None, None
        if ctx.needs_input_grad[1]:
            nch = m.conv2d_any_wgrad_chunks(B, Ho, Wo)
            part = torch.empty(nch, G, co, k * k, ci, device=xs.device, dtype=torch.float32)
            m.conv2d_any_wgrad(xs.data_ptr(), dy.data_ptr(), part.data_ptr(), G, B, H, W, ci, ci, co, k, pad,
                               _stream())
            dw = part.sum(0).view(G, co, k, k, ci).permute(0, 1, 4, 2, 3).contiguous()
        if want_b:
            db = dy.float().view(G, B * Ho * Wo, co).sum(1)
        return dx, dw, db, None, None


def _rows_bf16(x):
    return x.detach().to(torch.bfloat16).contiguous()


class HipLinearFn(torch.autograd.Function):
    """Grouped Linear on ``linear_g.hip``: x [G*B, K] (any float dtype), w the [G, N, K] fp32 view of the clients'
    rows (strides (ld, K, 1), read in place: no bf16 copy of the weights is made), b [G, N] (strides (ld, 1)) or
    None.  Returns bf16 [G*B, N]; the backward gives bf16 dx and fp32-accumulated fp32 dw / db."""

    @staticmethod
    def forward(ctx, x, w, b, G):
        m = ops.ext()
        M, K = x.shape
        N = w.shape[1]
        assert M % G == 0 and w.shape[0] == G and w.shape[2] == K and w.dtype == torch.float32
        ldw = w.stride(0)
        assert w.stride() == (ldw, K, 1), "HipLinearFn: w must be a [G, N, K] view of the clients' rows"
        ldb = 0
        if b is not None:
            ldb = b.stride(0)
            assert b.shape == (G, N) and b.stride() == (ldb, 1) and b.dtype == torch.float32
        xs = _rows_bf16(x)
        y = torch.empty(M, N, device=x.device, dtype=torch.bfloat16)
        m.linear_g_fwd(xs.data_ptr(), w.data_ptr(), ldw, b.data_ptr() if b is not None else 0, ldb, y.data_ptr(), G,
                       M // G, K, N, _stream())
        ctx.save_for_backward(xs, w)
        ctx.G, ctx.has_b = G, b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        m = ops.ext()
        xs, w = ctx.saved_tensors
        G = ctx.G
        M, K = xs.shape
        N, B = w.shape[1], M // G
        dy = _rows_bf16(gy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=xs.device, dtype=torch.bfloat16)
            m.linear_g_dgrad(dy.data_ptr(), w.data_ptr(), w.stride(0), dx.data_ptr(), G, B, K, N, _stream())
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw = torch.empty(G, N, K, device=xs.device, dtype=torch.float32)
            if ctx.has_b:
                db = torch.empty(G, N, device=xs.device, dtype=torch.float32)
            m.linear_g_wgrad(xs.data_ptr(), dy.data_ptr(), dw.data_ptr(), N * K, db.data_ptr() if ctx.has_b else 0, N,
                             G, B, K, N, _stream())
        return dx, dw, db, None


def _hip_linear_on():
    return os.environ.get("NIDT_B2D_LINEAR", "1") != "0"


class _Group:
    """The current step's grouping: G and the per-client parameter views {name: [G, *shape]}."""

    def __init__(self):
        self.G = 1
        self.params = {}


class GConv2d(nn.Module):
    def __init__(self, mod, name, grp):
        super().__init__()
        assert mod.stride == (1, 1) and mod.dilation == (1, 1) and mod.groups == 1, "GConv2d: stride-1 plain convs"
        assert mod.kernel_size[0] == mod.kernel_size[1] and mod.padding[0] == mod.padding[1]
        self.name, self.grp, self.pad = name, grp, int(mod.padding[0])
        self.has_b = mod.bias is not None

    def forward(self, x):
        P = self.grp.params
        w, b = P[self.name + ".weight"], (P[self.name + ".bias"] if self.has_b else None)
        if not x.is_cuda:  # CPU twin (tests of the grouped graph): one grouped library conv over the client axis
            G = self.grp.G
            N, C, H, W = x.shape
            xc = x.reshape(G, N // G, C, H, W).transpose(0, 1).reshape(N // G, G * C, H, W)
            y = F.conv2d(xc, w.reshape((-1,) + tuple(w.shape[2:])), b.reshape(-1) if b is not None else None,
                         padding=self.pad, groups=G)
            return y.view(N // G, G, -1, *y.shape[2:]).transpose(0, 1).reshape(N, -1, *y.shape[2:])
        return HipConv2dFn.apply(x, w, b, self.grp.G, self.pad)


class GLinear(nn.Module):
    def __init__(self, mod, name, grp):
        super().__init__()
        self.name, self.grp, self.has_b = name, grp, mod.bias is not None

    def forward(self, x):
        G, P = self.grp.G, self.grp.params
        w = P[self.name + ".weight"]
        if x.is_cuda and _hip_linear_on():
            return HipLinearFn.apply(x, w, P[self.name + ".bias"] if self.has_b else None, G)
        xg = x.reshape(G, x.shape[0] // G, x.shape[1])
        if not torch.is_autocast_enabled():
            xg = xg.to(w.dtype)
        if self.has_b:
            y = torch.baddbmm(P[self.name + ".bias"].unsqueeze(1), xg, w.transpose(1, 2))
        else:
            y = torch.bmm(xg, w.transpose(1, 2))
        return y.reshape(x.shape[0], w.shape[1])


def _hip_gn_on():
    return os.environ.get("NIDT_B2D_GN", "1") != "0"


def gn2d_ok(H, W, C, groups, pool):
    """The launcher's rule of ``gn2d_fwd`` / ``gn2d_bwd``: C / 8 a power of two up to 64, channels per group dividing
    8 or a multiple of 8, a register-resident sample (H W C <= 65536), even H and W under the pool."""
    nch = C // 8
    if C % 8 or nch < 1 or nch > 64 or nch & (nch - 1) or groups < 1 or C % groups:
        return False
    cg = C // groups
    return (8 % cg == 0 or cg % 8 == 0) and 0 < H * W * C <= 65536 and not (pool and (H % 2 or W % 2))


def pool2d_ok(H, W, C):
    """The launcher's rule of ``pool2d_fwd`` / ``pool2d_bwd``.  No measured rule on top of it
    (``profiles/r14_gn_pool.txt``): cnn_cifar10's 28 x 28 pool ran 3.9x / 1.28x faster forward + backward (100 x 16 /
    8 x 64); its 10 x 10 pool is launch-bound on both paths (about 0.02 ms forward) and the Python autograd function
    costs more host time than the framework op there, 0.76x at both sizes, yet the cnn_cifar10 step with both pools
    routed here took 0.861 / 0.964 of the step with ``NIDT_B2D_GN=0``."""
    return C % 8 == 0 and H % 2 == 0 and W % 2 == 0 and H > 0 and W > 0


def _affine_rows(gamma, beta):
    """gamma, beta [G, C] as fp32 tensors with unit channel stride and one common client stride (the views of the
    parameter rows are that already), and the stride."""
    ok = lambda a: a.dtype == torch.float32 and a.stride(1) == 1  # noqa: E731
    if not (ok(gamma) and ok(beta) and (gamma.shape[0] == 1 or gamma.stride(0) == beta.stride(0))):
        gamma, beta = gamma.float().contiguous(), beta.float().contiguous()
    return gamma, beta, (gamma.stride(0) if gamma.shape[0] > 1 else gamma.shape[1])


class HipGroupNormFn(torch.autograd.Function):
    """GroupNorm with a per-client affine, optional ReLU and optional 2 x 2 max-pool on ``gn_pool.hip``:
    x [G*B, C, H, W] (any strides), gamma / beta the [G, C] fp32 views of the clients' rows.  Returns the bf16
    channels-last result as an NCHW view; the backward gives bf16 dx and fp32 dgamma / dbeta (the per-sample
    partials summed over each client's samples in a fixed order by ``gn_param_grads``)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, groups, eps, relu, pool):
        m = ops.ext()
        N, C, H, W = x.shape
        assert N % G == 0 and gamma.shape == (G, C) and beta.shape == (G, C)
        xs = _aligned16(_nhwc_bf16(x))
        ga, be, ld = _affine_rows(gamma.detach(), beta.detach())
        y = torch.empty((N, H // 2, W // 2, C) if pool else (N, H, W, C), device=x.device, dtype=torch.bfloat16)
        train = any(ctx.needs_input_grad[:3])
        stats = torch.empty(N, groups, 2, device=x.device, dtype=torch.float32) if train else None
        m.gn2d_fwd(xs.data_ptr(), ga.data_ptr(), be.data_ptr(), ld, y.data_ptr(), stats.data_ptr() if train else 0, N,
                   N // G, H, W, C, groups, float(eps), int(relu), int(pool), _stream())
        if train:
            ctx.save_for_backward(xs, stats, ga, be)
        ctx.cfg = (G, groups, ld, int(relu), int(pool))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        m = ops.ext()
        xs, stats, ga, be = ctx.saved_tensors
        G, groups, ld, relu, pool = ctx.cfg
        N, H, W, C = xs.shape
        dy = _aligned16(_nhwc_bf16(gy))
        dt = torch.empty_like(xs)
        part = torch.empty(N, C, 2, device=xs.device, dtype=torch.float32)
        m.gn2d_bwd(dy.data_ptr(), xs.data_ptr(), stats.data_ptr(), ga.data_ptr(), be.data_ptr(), ld, dt.data_ptr(),
                   part.data_ptr(), N, N // G, H, W, C, groups, relu, pool, _stream())
        gr = torch.empty(G, 2, C, device=xs.device, dtype=torch.float32)  # (dgamma, dbeta) of each client
        m.gn_param_grads(part.data_ptr(), G, N // G, C, gr.data_ptr(), 2 * C, 0, C, _stream())
        return dt.permute(0, 3, 1, 2), gr[:, 0], gr[:, 1], None, None, None, None, None


class HipMaxPool2dFn(torch.autograd.Function):
    """2 x 2 stride-2 max-pool on ``gn_pool.hip``: x [N, C, H, W] (any strides) -> bf16 channels-last result as an
    NCHW view; the backward recomputes the argmax from the saved input (first maximum in (row, column) order)."""

    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        xs = _aligned16(_nhwc_bf16(x))
        y = torch.empty(N, H // 2, W // 2, C, device=x.device, dtype=torch.bfloat16)
        ops.ext().pool2d_fwd(xs.data_ptr(), y.data_ptr(), N, H, W, C, _stream())
        ctx.save_for_backward(xs)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        xs, = ctx.saved_tensors
        N, H, W, C = xs.shape
        dy = _aligned16(_nhwc_bf16(gy))
        dx = torch.empty_like(xs)
        ops.ext().pool2d_bwd(dy.data_ptr(), xs.data_ptr(), dx.data_ptr(), N, H, W, C, _stream())
        return dx.permute(0, 3, 1, 2)


class GGroupNorm(nn.Module):
    """GroupNorm twin; ``relu`` / ``pool``: the ReLU (an ``nn.ReLU``, kept for its ``inplace``) and the
    ``MaxPool2d(2, 2)`` that ``grouped_model`` absorbed into it."""

    def __init__(self, mod, name, grp, relu=None, pool=False):
        super().__init__()
        self.name, self.grp = name, grp
        self.num_groups, self.eps, self.affine = mod.num_groups, mod.eps, mod.affine
        self.relu, self.relu_inplace, self.pool = relu is not None, bool(relu is not None and relu.inplace), bool(pool)

    def forward(self, x):
        G = self.grp.G
        P = self.grp.params
        if x.is_cuda and self.affine and x.dim() == 4 and _hip_gn_on() and \
                gn2d_ok(x.shape[2], x.shape[3], x.shape[1], self.num_groups, self.pool):
            return HipGroupNormFn.apply(x, P[self.name + ".weight"], P[self.name + ".bias"], G, self.num_groups,
                                        self.eps, self.relu, self.pool)
        y = F.group_norm(x, self.num_groups, None, None, self.eps)
        if self.affine:
            N, C = y.shape[:2]
            w = P[self.name + ".weight"].view((G, 1, C) + (1,) * (y.dim() - 2))
            b = P[self.name + ".bias"].view((G, 1, C) + (1,) * (y.dim() - 2))
            y = (y.view((G, N // G) + tuple(y.shape[1:])) * w + b).view(y.shape)
        if self.relu:
            y = F.relu(y, inplace=self.relu_inplace)
        return F.max_pool2d(y, 2, 2) if self.pool else y


class GMaxPool2d(nn.Module):
    def forward(self, x):
        if x.is_cuda and x.dim() == 4 and _hip_gn_on() and pool2d_ok(x.shape[2], x.shape[3], x.shape[1]):
            return HipMaxPool2dFn.apply(x)
        return F.max_pool2d(x, 2, 2)


def _pool22(mod):
    """An ``nn.MaxPool2d(2, 2)`` with padding 0, dilation 1, no ``ceil_mode`` and no indices."""
    pair = lambda v, a: v == a or v == (a, a)  # noqa: E731
    return (isinstance(mod, nn.MaxPool2d) and pair(mod.kernel_size, 2) and pair(mod.stride, 2)
            and pair(mod.padding, 0) and pair(mod.dilation, 1) and not mod.ceil_mode and not mod.return_indices)


_SWAP = {nn.Conv2d: GConv2d, nn.Linear: GLinear, nn.GroupNorm: GGroupNorm}


def supports(model):
    """True when every parametrised layer has a grouped twin (stride-1 plain Conv2d, Linear, GroupNorm)."""
    for mod in model.modules():
        if isinstance(mod, nn.Conv2d):
            if mod.stride != (1, 1) or mod.dilation != (1, 1) or mod.groups != 1 or \
                    mod.kernel_size[0] != mod.kernel_size[1] or mod.padding[0] != mod.padding[1] or \
                    mod.padding_mode != "zeros":
                return False
        elif len(list(mod.parameters(recurse=False))) and type(mod) not in _SWAP:
            return False
    return True


def grouped_model(model):
    """(deep copy of ``model`` with the grouped twins swapped in, its _Group holder)."""
    grp = _Group()
    gm = copy.deepcopy(model)

    def swap(parent, prefix):
        kids = list(parent.named_children())
        absorbed = set()
        for i, (cname, child) in enumerate(kids):
            full = prefix + cname
            cls = _SWAP.get(type(child))
            if cname in absorbed:  # a ReLU / MaxPool2d that the GroupNorm before it runs: the index stays
                setattr(parent, cname, nn.Identity())
            elif cls is GGroupNorm:
                relu, pool = None, False
                if isinstance(parent, nn.Sequential) and i + 1 < len(kids) and type(kids[i + 1][1]) is nn.ReLU:
                    relu = kids[i + 1][1]
                    pool = i + 2 < len(kids) and _pool22(kids[i + 2][1])
                    absorbed.update(k for k, _ in kids[i + 1:i + 3 if pool else i + 2])
                setattr(parent, cname, GGroupNorm(child, full, grp, relu, pool))
            elif cls is not None:
                setattr(parent, cname, cls(child, full, grp))
            elif _pool22(child):
                setattr(parent, cname, GMaxPool2d())
            else:
                swap(child, full + ".")
    swap(gm, "")
    for p in gm.parameters():  # the twins read the clients' rows; no module parameters are left
        raise AssertionError("grouped_model: parameter left in the grouped copy")
    return gm, grp
