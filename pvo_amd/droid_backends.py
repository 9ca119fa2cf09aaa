"""`droid_backends` — the reference's native op surface, backed by libpvo_hip.so.

Mirrors the pybind module of the reference (VO_Module/src/droid.cpp:234-247):
same function names, positional argument order, in-place semantics and error
behaviour (RuntimeError "<name> must be contiguous", droid.cpp:83-84).  Each
function forwards raw device pointers + sizes + torch's CURRENT HIP stream to the
C ABI of include/pvo_hip.h.  There is no CPU / PyTorch fallback: CPU tensors, a
missing shared library or a failing launch raise.

A maintainer of the reference replaces `import droid_backends` with
`from pvo_amd import droid_backends`.
"""
import ctypes
import itertools

import torch

from . import _lib
from ._lib import PvoHipError, check

_DT = {torch.float32: _lib.PVO_F32, torch.float16: _lib.PVO_F16,
       torch.bfloat16: _lib.PVO_BF16, torch.float64: _lib.PVO_F64}

_ws_cache = {}


def _contig(t, name):
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)  # droid.cpp:83 CHECK_CONTIGUOUS


def _dev(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise PvoHipError("droid_backends (MI355X build) needs device tensors; got a CPU tensor "
                              "(there is no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise PvoHipError("all tensors must live on the same device")
    return dev


class _PinnedRing:
    """One persistent page-locked staging buffer per process.  `tensor.pin_memory()` per call is a fresh page-locked
    allocation whenever the caching host allocator cannot recycle a block (its blocks are only recycled once the copy
    that used them has completed, and the host runs ahead of the GPU), i.e. a hipHostMalloc - milliseconds, and a
    device-wide lock - in the middle of the update loop.  Small index lists are copied into this ring instead; a quarter
    of the ring is reused only after the copies issued from it have completed (an event per quarter)."""

    def __init__(self, nbytes=1 << 20, pin=True):
        buf = torch.empty(nbytes, dtype=torch.uint8)
        self.buf = buf.pin_memory() if pin else buf
        self.nbytes, self.quarter = nbytes, nbytes // 4
        self.off = 0                  # next free byte, always inside quarter `self.q`
        self.q = 0                    # the quarter allocations currently come from (tracked, not derived from `off`:
        self.events = [None] * 4      # an allocation that ends exactly on a boundary leaves `off` in the next quarter's range)

    def _record(self, device):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        return ev

    def take(self, n, device):
        n = (n + 15) & ~15
        if n > self.quarter:
            return None
        if self.off + n > (self.q + 1) * self.quarter:        # does not fit in what is left of the current quarter: move on
            self.events[self.q] = self._record(device)        # copies issued from the quarter being left
            self.q = (self.q + 1) % 4
            self.off = self.q * self.quarter
            if self.events[self.q] is not None:               # copies issued from this quarter one lap ago
                self.events[self.q].synchronize()
                self.events[self.q] = None
        seg = self.buf[self.off:self.off + n]
        self.off += n
        return seg


_ring = None


def to_device_async(values, dtype, device):
    """host sequence -> device tensor through the pinned staging ring and an asynchronous copy: unlike
    torch.tensor(values, device=...) this neither drains the stream nor allocates page-locked memory"""
    global _ring
    t = values.to(dtype) if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=dtype)
    device = torch.device(device)
    if device.type != "cuda" or t.numel() == 0:
        return t.to(device)
    if _ring is None:
        _ring = _PinnedRing()
    nbytes = t.numel() * t.element_size()
    seg = _ring.take(nbytes, device)
    if seg is None:                                           # larger than a quarter of the ring: rare, one-off
        return t.pin_memory().to(device, non_blocking=True)
    stage = seg[:nbytes].view(dtype).view(t.shape)
    stage.copy_(t)
    out = torch.empty(t.shape, dtype=dtype, device=device)
    out.copy_(stage, non_blocking=True)
    return out


def to_device_packed(parts, device):
    """several host index lists -> device tensors in ONE staged upload: parts = [(values, dtype), ...]; returns one
    tensor per part, each a 16-byte aligned view of a single device buffer.  An edge-set change needs about ten small
    index tables (edge lists, slots, segment CSR, damping rows ...); as separate copies each is a ~4 us blit on the
    stream, which at 200 keyframes/s is worth counting."""
    device = torch.device(device)
    ts = [(v.to(dt) if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=dt)).reshape(-1) for v, dt in parts]
    if device.type != "cuda":
        return [t.to(device) for t in ts]
    offs, total = [], 0
    for t in ts:
        offs.append(total)
        total += (t.numel() * t.element_size() + 15) & ~15
    if total == 0:
        return [t.to(device) for t in ts]
    host = torch.empty(total, dtype=torch.uint8)
    for t, o in zip(ts, offs):
        if t.numel():
            host[o:o + t.numel() * t.element_size()].view(t.dtype).copy_(t)
    dev = to_device_async(host, torch.uint8, device)
    return [dev[o:o + t.numel() * t.element_size()].view(t.dtype) for t, o in zip(ts, offs)]


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def _dtype_code(t, what):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise PvoHipError("%s: unsupported dtype %s" % (what, t.dtype))


def _long(t, name):
    if t.dtype != torch.int64:
        raise PvoHipError("%s must be int64 (the reference reads it through packed_accessor32<long>)" % name)


def _f32(t, name):
    if t.dtype != torch.float32:
        raise PvoHipError("%s must be float32" % name)


def _workspace(dev, nbytes):
    key = (dev.index if dev.index is not None else torch.cuda.current_device())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=dev)
        _ws_cache[key] = buf
    return buf


# --------------------------------------------------------------------------- correlation
def corr_index_forward(volume, coords, radius):
    """droid.cpp:167-175. volume [N,h1,w1,h2,w2], coords [N,2,h1,w1] f32 -> [corr [N,2r+1,2r+1,h1,w1]]."""
    _contig(volume, "volume"); _contig(coords, "coords")
    dev = _dev(volume, coords)
    _f32(coords, "coords")
    N, h1, w1, h2, w2 = volume.shape
    rd = 2 * radius + 1
    corr = torch.empty((N, rd, rd, h1, w1), dtype=volume.dtype, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.pvo_corr_index_forward(_ptr(volume), _ptr(coords), _ptr(corr), N, h1, w1, h2, w2,
                                         radius, _dtype_code(volume, "volume"), _stream(dev)),
              "corr_index_forward")
    return [corr]


def corr_index_backward(volume, coords, corr_grad, radius):
    """droid.cpp:177-188 -> [volume_grad] (same shape/dtype as volume)."""
    _contig(volume, "volume"); _contig(coords, "coords"); _contig(corr_grad, "corr_grad")
    dev = _dev(volume, coords, corr_grad)
    _f32(coords, "coords")
    if corr_grad.dtype != volume.dtype:
        raise PvoHipError("corr_grad dtype must match volume dtype")
    N, h1, w1, h2, w2 = volume.shape
    volume_grad = torch.empty_like(volume)
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.pvo_corr_index_backward(_ptr(coords), _ptr(corr_grad), _ptr(volume_grad),
                                          N, h1, w1, h2, w2, radius,
                                          _dtype_code(volume, "volume"), _stream(dev)),
              "corr_index_backward")
    return [volume_grad]


def corr_pyramid_lookup(pyramid, coords, radius, channels_last=False, slots=None):
    """All levels of CorrBlock.__call__ (modules/corr.py:40-50) in one launch.

    pyramid: list of level tensors [N,h1,w1,h2>>l,w2>>l]; coords [N,h1,w1,2] f32
    -> [N, L*(2r+1)^2, h1, w1]; with channels_last=True the same tensor is returned with
    channels-last strides (stored [N,h1,w1,L*(2r+1)^2]), ready for NHWC convolutions.
    Not part of the reference surface: it is what the Python loop + torch.cat computes, fused."""
    dev = _dev(coords, *pyramid)
    _contig(coords, "coords"); _f32(coords, "coords")
    for lv in pyramid:
        _contig(lv, "volume")
    NV, h1, w1, h2, w2 = pyramid[0].shape
    L = len(pyramid)
    for l, lv in enumerate(pyramid):
        if tuple(lv.shape) != (NV, h1, w1, h2 >> l, w2 >> l) or lv.dtype != pyramid[0].dtype:
            raise PvoHipError("pyramid level %d has shape %s, expected %s"
                              % (l, tuple(lv.shape), (NV, h1, w1, h2 >> l, w2 >> l)))
    N = coords.shape[0]
    if slots is None:
        if N != NV:
            raise PvoHipError("coords has %d edges but the pyramid holds %d volumes" % (N, NV))
    elif slots.dtype != torch.int32 or slots.numel() != N or not slots.is_cuda:
        raise PvoHipError("slots must be a device int32 tensor with one entry per edge")
    rd = 2 * radius + 1
    if channels_last:
        out = torch.empty((N, h1, w1, L * rd * rd), dtype=pyramid[0].dtype, device=dev).permute(0, 3, 1, 2)
    else:
        out = torch.empty((N, L * rd * rd, h1, w1), dtype=pyramid[0].dtype, device=dev)
    ptrs = (ctypes.c_void_p * L)(*[lv.data_ptr() if lv.numel() else 0 for lv in pyramid])
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.pvo_corr_pyramid_lookup(ptrs, _ptr(coords), _ptr(out), N, h1, w1, h2, w2, L, radius,
                                          _dtype_code(pyramid[0], "volume"), 1 if channels_last else 0,
                                          _ptr(slots), NV, _stream(dev)),
              "corr_pyramid_lookup")
    return out


def tiled_level_shape(ht, wd, level):
    """trailing dims (th, tw, 8, 8) of level `level` of an 8x8-tiled pyramid over an ht x wd target image"""
    return (((ht >> level) + 7) // 8, ((wd >> level) + 7) // 8, 8, 8)


def tiled_supported(ht, wd, dtype):
    return dtype in (torch.float16, torch.bfloat16) and wd >= 8 and ht >= 8


def corr_build_tiled(fmap1, fmap2, out, out_slots):
    """pvo_corr_build_tiled: edge n -> slot out_slots[n] of the tiled level tensors `out`
    ([slots, H, W, th, tw, 8, 8] per level); fmap1/fmap2 [N,H,W,C] channels-last 16-bit."""
    _contig(fmap1, "fmap1"); _contig(fmap2, "fmap2")
    dev = _dev(fmap1, fmap2, out_slots, *out)
    N, H, W, C = fmap1.shape
    if fmap1.shape != fmap2.shape or fmap1.dtype != fmap2.dtype or len(out) != 4:
        raise PvoHipError("corr_build_tiled: fmap mismatch or not 4 levels")
    for l, lv in enumerate(out):
        if tuple(lv.shape[1:]) != (H, W) + tiled_level_shape(H, W, l) or lv.dtype != fmap1.dtype or not lv.is_contiguous():
            raise PvoHipError("corr_build_tiled: level %d has shape %s" % (l, tuple(lv.shape)))
    if out_slots.dtype != torch.int32 or out_slots.numel() != N:
        raise PvoHipError("corr_build_tiled: out_slots must be device int32, one per edge")
    ptrs = (ctypes.c_void_p * 4)(*[lv.data_ptr() for lv in out])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_corr_build_tiled(_ptr(fmap1), _ptr(fmap2), ptrs, N, C, H, W, _dtype_code(fmap1, "fmap"),
                                               _ptr(out_slots), _stream(dev)), "corr_build_tiled")
    return out


def corr_build_tiled_rows(fmaps1, fmaps2, rows1, rows2, out, out_slots):
    """pvo_corr_build_tiled_rows: corr_build_tiled straight from frame buffers - edge n correlates frame rows1[n] of fmaps1 with
    frame rows2[n] of fmaps2 ([F,H,W,C] channels-last 16-bit; rows1 / rows2 / out_slots device int32 [N]).  The values of the
    tables are not checked: rows inside the buffers are the caller's business."""
    _contig(fmaps1, "fmaps1"); _contig(fmaps2, "fmaps2")
    dev = _dev(fmaps1, fmaps2, rows1, rows2, out_slots, *out)
    _, H, W, C = fmaps1.shape
    N = rows1.numel()
    if fmaps1.shape[1:] != fmaps2.shape[1:] or fmaps1.dtype != fmaps2.dtype or len(out) != 4:
        raise PvoHipError("corr_build_tiled_rows: fmap mismatch or not 4 levels")
    for l, lv in enumerate(out):
        if tuple(lv.shape[1:]) != (H, W) + tiled_level_shape(H, W, l) or lv.dtype != fmaps1.dtype or not lv.is_contiguous():
            raise PvoHipError("corr_build_tiled_rows: level %d has shape %s" % (l, tuple(lv.shape)))
    for t, name in ((rows1, "rows1"), (rows2, "rows2"), (out_slots, "out_slots")):
        if t.dtype != torch.int32 or t.numel() != N or not t.is_contiguous():
            raise PvoHipError("corr_build_tiled_rows: %s must be device int32, one per edge" % name)
    ptrs = (ctypes.c_void_p * 4)(*[lv.data_ptr() for lv in out])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_corr_build_tiled_rows(_ptr(fmaps1), _ptr(fmaps2), _ptr(rows1), _ptr(rows2), ptrs, N, C, H, W,
                                                    _dtype_code(fmaps1, "fmap"), _ptr(out_slots), _stream(dev)), "corr_build_tiled_rows")
    return out


def corr_pyramid_lookup_tiled(pyramid, coords, channels_last=False, slots=None):
    """radius-3 lookup of all levels of an 8x8-tiled pyramid (see corr_build_tiled); same result as
    corr_pyramid_lookup on the row-major pyramid."""
    dev = _dev(coords, *pyramid)
    _contig(coords, "coords"); _f32(coords, "coords")
    NV, h1, w1 = pyramid[0].shape[:3]
    th0, tw0 = pyramid[0].shape[3:5]
    L = len(pyramid)
    N = coords.shape[0]
    if slots is None:
        if N != NV:
            raise PvoHipError("coords has %d edges but the pyramid holds %d volumes" % (N, NV))
    elif slots.dtype != torch.int32 or slots.numel() != N or not slots.is_cuda:
        raise PvoHipError("slots must be a device int32 tensor with one entry per edge")
    for l, lv in enumerate(pyramid):
        if tuple(lv.shape) != (NV, h1, w1) + tiled_level_shape(h1, w1, l) or not lv.is_contiguous():
            raise PvoHipError("tiled pyramid level %d has shape %s" % (l, tuple(lv.shape)))
    if channels_last:
        out = torch.empty((N, h1, w1, L * 49), dtype=pyramid[0].dtype, device=dev).permute(0, 3, 1, 2)
    else:
        out = torch.empty((N, L * 49, h1, w1), dtype=pyramid[0].dtype, device=dev)
    ptrs = (ctypes.c_void_p * L)(*[lv.data_ptr() for lv in pyramid])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_corr_pyramid_lookup_tiled(ptrs, _ptr(coords), _ptr(out), N, h1, w1, h1, w1, L,
                                                        _dtype_code(pyramid[0], "volume"), 1 if channels_last else 0,
                                                        _ptr(slots), NV, _stream(dev)), "corr_pyramid_lookup_tiled")
    return out


def corr_encoder_weights(weight, dtype):
    """Conv2d(196,128,1) filter [128,196,1,1] -> the zero-padded [128,224] matrix pvo_corr_lookup_encode_tiled reads"""
    if tuple(weight.shape[:2]) != (128, 196):
        raise PvoHipError("corr_encoder_weights: filter must be [128,196,1,1]")
    w = torch.zeros(128, 224, dtype=dtype, device=weight.device)
    w[:, :196] = weight.detach().reshape(128, 196).to(dtype)
    return w


def corr_lookup_encode_tiled(pyramid, coords, enc_weight, enc_bias, slots=None):
    """relu(W corr + b) with corr = the radius-3 lookup of the 8x8-tiled pyramid, in one kernel
    -> [N,128,h1,w1] stored channels-last (the input of corr_encoder[2])."""
    dev = _dev(coords, enc_weight, enc_bias, *pyramid)
    _contig(coords, "coords"); _f32(coords, "coords")
    NV, h1, w1 = pyramid[0].shape[:3]
    N = coords.shape[0]
    if len(pyramid) != 4:
        raise PvoHipError("corr_lookup_encode_tiled: 4 levels required")
    if slots is None:
        if N != NV:
            raise PvoHipError("coords has %d edges but the pyramid holds %d volumes" % (N, NV))
    elif slots.dtype != torch.int32 or slots.numel() != N or not slots.is_cuda:
        raise PvoHipError("slots must be a device int32 tensor with one entry per edge")
    for l, lv in enumerate(pyramid):
        if tuple(lv.shape) != (NV, h1, w1) + tiled_level_shape(h1, w1, l) or not lv.is_contiguous():
            raise PvoHipError("tiled pyramid level %d has shape %s" % (l, tuple(lv.shape)))
    if tuple(enc_weight.shape) != (128, 224) or enc_weight.dtype != pyramid[0].dtype or not enc_weight.is_contiguous():
        raise PvoHipError("enc_weight must be the [128,224] tensor of corr_encoder_weights in the volume dtype")
    out = torch.empty((N, h1, w1, 128), dtype=pyramid[0].dtype, device=dev).permute(0, 3, 1, 2)
    ptrs = (ctypes.c_void_p * 4)(*[lv.data_ptr() for lv in pyramid])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_corr_lookup_encode_tiled(ptrs, _ptr(coords), _ptr(enc_weight), _bias(enc_bias, 128, "enc_bias"),
                                                       _ptr(out), N, h1, w1, _dtype_code(pyramid[0], "volume"),
                                                       _ptr(slots), NV, _stream(dev)), "corr_lookup_encode_tiled")
    return out


def altcorr_forward(fmap1, fmap2, coords, radius):
    """droid.cpp:190-200. fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C], coords [B,S,H1,W1,2] -> [corr [B,S,(2r+1)^2,H1,W1]]"""
    _contig(fmap1, "fmap1"); _contig(fmap2, "fmap2"); _contig(coords, "coords")
    dev = _dev(fmap1, fmap2, coords)
    _f32(coords, "coords")
    if fmap1.dtype != torch.float32 or fmap2.dtype != torch.float32:
        raise PvoHipError("altcorr_forward: float32 features only (AltCorrBlock casts with .float(), corr.py:120)")
    B, H1, W1, C = fmap1.shape
    _, H2, W2, _ = fmap2.shape
    S = coords.shape[1]
    rd = 2 * radius + 1
    corr = torch.empty(B, S, rd * rd, H1, W1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_altcorr_forward(_ptr(fmap1), _ptr(fmap2), _ptr(coords), _ptr(corr), B, S, H1, W1, H2, W2, C,
                                              radius, _lib.PVO_F32, _stream(dev)), "altcorr_forward")
    return [corr]


def altcorr_backward(fmap1, fmap2, coords, corr_grad, radius):
    """droid.cpp:202-214 -> [fmap1_grad, fmap2_grad, coords_grad (zeros, as altcorr_kernel.cu:340)]"""
    for t, n in ((fmap1, "fmap1"), (fmap2, "fmap2"), (coords, "coords"), (corr_grad, "corr_grad")):
        _contig(t, n)
    dev = _dev(fmap1, fmap2, coords, corr_grad)
    if any(t.dtype != torch.float32 for t in (fmap1, fmap2, coords, corr_grad)):
        raise PvoHipError("altcorr_backward: float32 only (altcorr_kernel.cu:345)")
    B, H1, W1, C = fmap1.shape
    _, H2, W2, _ = fmap2.shape
    S = coords.shape[1]
    g1, g2 = torch.empty_like(fmap1), torch.empty_like(fmap2)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_altcorr_backward(_ptr(fmap1), _ptr(fmap2), _ptr(coords), _ptr(corr_grad), _ptr(g1), _ptr(g2),
                                               B, S, H1, W1, H2, W2, C, radius, _lib.PVO_F32, _stream(dev)),
              "altcorr_backward")
    return [g1, g2, torch.zeros(B, S, H1, W1, 2, dtype=torch.float32, device=dev)]


def corr_build(fmap1, fmap2, num_levels=4, channels_last=False, out=None, out_slots=None):
    """CorrBlock.corr + the avg-pool pyramid (modules/corr.py:24-38,63-71) in one launch.

    fmap1, fmap2: [N,C,H,W] (channels_last=False) or [N,H,W,C] (channels_last=True).
    Returns the pyramid: level l is [N,H,W,H>>l,W>>l] in the feature dtype.
    out / out_slots: write edge n into slot out_slots[n] (device int32) of the existing level tensors `out`."""
    _contig(fmap1, "fmap1"); _contig(fmap2, "fmap2")
    dev = _dev(fmap1, fmap2)
    if fmap1.shape != fmap2.shape or fmap1.dtype != fmap2.dtype:
        raise PvoHipError("corr_build: fmap1/fmap2 shape or dtype mismatch")
    if channels_last:
        N, H, W, C = fmap1.shape
    else:
        N, C, H, W = fmap1.shape
    if out is not None:
        levels = out
        if out_slots is None or out_slots.dtype != torch.int32 or out_slots.numel() != N:
            raise PvoHipError("corr_build: out needs out_slots (device int32, one per edge)")
    else:
        levels = [torch.empty((N, H, W, H >> l, W >> l), dtype=fmap1.dtype, device=dev) for l in range(num_levels)]
    ptrs = (ctypes.c_void_p * num_levels)(*[lv.data_ptr() if lv.numel() else 0 for lv in levels])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_corr_build(_ptr(fmap1), _ptr(fmap2), ptrs, N, C, H, W, num_levels,
                                         _dtype_code(fmap1, "fmap"), 1 if channels_last else 0, _ptr(out_slots), _stream(dev)),
              "corr_build")
    return levels


# --------------------------------------------------------------------------- reprojection family
def frame_distance(poses, disps, intrinsics, ii, jj, beta):
    """droid.cpp:117-133 -> dist [M]."""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj")):
        _contig(t, n)
    dev = _dev(poses, disps, intrinsics, ii, jj)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics"); _long(ii, "ii"); _long(jj, "jj")
    M = ii.shape[0]
    dist = torch.empty(M, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_frame_distance(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj),
                                             _ptr(dist), M, disps.shape[1], disps.shape[2], float(beta),
                                             _stream(dev)), "frame_distance")
    return dist


def frame_distance_bidirectional(poses, disps, intrinsics, ii, jj, beta):
    """0.5 * (frame_distance(ii, jj) + frame_distance(jj, ii)) - DepthVideo.distance's bidirectional metric
    (depth_video.py:183-193) - in one launch, bit-identical to the two-call formulation -> dist [M]."""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj")):
        _contig(t, n)
    dev = _dev(poses, disps, intrinsics, ii, jj)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics"); _long(ii, "ii"); _long(jj, "jj")
    M = ii.shape[0]
    dist = torch.empty(M, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_frame_distance_bidirectional(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj),
                                                           _ptr(dist), M, disps.shape[1], disps.shape[2], float(beta),
                                                           _stream(dev)), "frame_distance_bidirectional")
    return dist


def projmap(poses, disps, intrinsics, ii, jj):
    """droid.cpp:136-151 -> [coords [E,ht,wd,3], valid [E,ht,wd,1]]."""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj")):
        _contig(t, n)
    dev = _dev(poses, disps, intrinsics, ii, jj)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics"); _long(ii, "ii"); _long(jj, "jj")
    E, ht, wd = ii.shape[0], disps.shape[1], disps.shape[2]
    coords = torch.empty(E, ht, wd, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(E, ht, wd, 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_projmap(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj),
                                      _ptr(coords), _ptr(valid), E, ht, wd, _stream(dev)), "projmap")
    return [coords, valid]


def iproj(poses, disps, intrinsics):
    """droid.cpp:154-163 -> points [N,ht,wd,3]."""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics")):
        _contig(t, n)
    dev = _dev(poses, disps, intrinsics)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics")
    N, ht, wd = disps.shape
    pts = torch.empty(N, ht, wd, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_iproj(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(pts), N, ht, wd,
                                    _stream(dev)), "iproj")
    return pts


def depth_filter(poses, disps, intrinsics, ix, thresh):
    """droid.cpp:217-231 -> counter [N,ht,wd]."""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ix, "ix"), (thresh, "thresh")):
        _contig(t, n)
    dev = _dev(poses, disps, intrinsics, ix, thresh)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics"); _long(ix, "ix"); _f32(thresh, "thresh")
    N, (nf, ht, wd) = ix.shape[0], disps.shape
    counter = torch.empty(N, ht, wd, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_depth_filter(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ix), _ptr(thresh),
                                           _ptr(counter), N, nf, ht, wd, _stream(dev)), "depth_filter")
    return counter


def map_points(poses, disps, intrinsics, ix, thresh, images=None, img_stride=8, img_offset=3, labels=None, label_div=1, reject=None,
               min_votes=2, mean_frac=0.5, capacity=None):
    """The filtered point cloud of keyframes ix (include/pvo_hip.h pvo_map_points; the reference's viewer loop,
    visualization.py:92-107,127-129): pixels confirmed by >= min_votes neighbouring keyframes (depth_filter's votes for thresh [N])
    whose inverse depth exceeds mean_frac of their frame's mean, back-projected into the world, compacted in the order of ix and, inside
    a frame, in raster order.  images uint8 [nframes,3,IH,IW] (BGR) give colours from [img_offset::img_stride] in both directions,
    labels int32 [nframes,LH,LW] labels at (y // label_div, x // label_div), reject (bool / uint8, shaped like labels; labels' shape
    if both are given) drops the pixels of its nonzero cells.

    Returns a dict: xyz f32 [n,3], rgba uint8 [n,4] (a = votes; rgb 0 without images), src int32 [n,2] = (frame, pixel), label
    int32 [n] (only with labels), frame_start int32 [N+1] (frame_start[N] = the number of points found).
    capacity=None allocates the upper bound N*ht*wd, reads the total back ONCE - the call's one host synchronisation - and returns
    the tensors sliced to it.  An explicit capacity returns the unsliced [capacity, ...] buffers and never synchronises: points
    beyond it are dropped, which frame_start[N] > capacity tells."""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ix, "ix"), (thresh, "thresh"), (images, "images"),
                 (labels, "labels"), (reject, "reject")):
        if t is not None:
            _contig(t, n)
    dev = _dev(poses, disps, intrinsics, ix, thresh, images, labels, reject)
    _long(ix, "ix"); _f32(thresh, "thresh"); _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics")
    N, (nf, ht, wd) = ix.shape[0], disps.shape
    if thresh.shape[0] != N:
        raise PvoHipError("map_points: thresh must have one entry per exported frame")
    a = _lib.MapPointsArgs()
    if images is not None:
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[0] < nf or images.shape[1] != 3:
            raise PvoHipError("map_points: images must be uint8 [nframes,3,IH,IW]")
        a.images, a.IH, a.IW, a.img_stride, a.img_offset = _ptr(images), images.shape[2], images.shape[3], int(img_stride), int(img_offset)
    if labels is not None:
        labels = labels.reshape(labels.shape[0], labels.shape[-2], labels.shape[-1])
        if labels.dtype != torch.int32 or labels.shape[0] < nf:
            raise PvoHipError("map_points: labels must be int32 [nframes,LH,LW]")
    if reject is not None:
        reject = reject.reshape(reject.shape[0], reject.shape[-2], reject.shape[-1])
        if reject.dtype == torch.bool:
            reject = reject.view(torch.uint8)
        if reject.dtype != torch.uint8 or reject.shape[0] < nf or (labels is not None and reject.shape[1:] != labels.shape[1:]):
            raise PvoHipError("map_points: reject must be bool / uint8 [nframes,LH,LW], the shape of labels")
    grid = labels if labels is not None else reject
    if grid is not None:
        a.labels, a.reject, a.LH, a.LW, a.label_div = _ptr(labels), _ptr(reject), grid.shape[1], grid.shape[2], int(label_div)
    cap = N * ht * wd if capacity is None else int(capacity)
    xyz = torch.empty(cap, 3, dtype=torch.float32, device=dev)
    rgba = torch.empty(cap, 4, dtype=torch.uint8, device=dev)
    src = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    label = torch.empty(cap, dtype=torch.int32, device=dev) if labels is not None else None
    frame_start = torch.empty(N + 1, dtype=torch.int32, device=dev)
    out = {"xyz": xyz, "rgba": rgba, "src": src, "frame_start": frame_start}
    if label is not None:
        out["label"] = label
    map_points_into(a, poses, disps, intrinsics, ix, thresh, out, min_votes, mean_frac)
    if capacity is None:
        n = int(frame_start[N].item())                  # the one synchronisation
        for k in ("xyz", "rgba", "src", "label"):
            if k in out:
                out[k] = out[k][:n]
    return out


def map_points_into(a, poses, disps, intrinsics, ix, thresh, out, min_votes=2, mean_frac=0.5):
    """map_points' native call on caller-owned output buffers (out: xyz [capacity,3], frame_start [N+1], optional rgba / label / src;
    the capacity is xyz's first dimension); `a`: a _lib.MapPointsArgs with the image / label / reject fields already set.  Buffers
    keep whatever they held beyond the points written.  No allocation beyond the cached workspace, no synchronisation."""
    dev = poses.device
    N, (nf, ht, wd) = ix.shape[0], disps.shape
    a.poses, a.disps, a.intrinsics, a.ix, a.thresh = _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ix), _ptr(thresh)
    a.N, a.nframes, a.ht, a.wd, a.min_votes, a.mean_frac = N, nf, ht, wd, int(min_votes), float(mean_frac)
    a.capacity = out["xyz"].shape[0]
    a.xyz, a.rgba, a.label, a.src = _ptr(out["xyz"]), _ptr(out.get("rgba")), _ptr(out.get("label")), _ptr(out.get("src"))
    a.frame_start = ctypes.c_void_p(out["frame_start"].data_ptr())
    lib = _lib.load()
    nbytes = lib.pvo_map_points_workspace_bytes(N, ht, wd)
    ws = _workspace(dev, nbytes)
    with torch.cuda.device(dev):
        check(lib.pvo_map_points(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "map_points")


def _panoptic(what, dev, shape, nframes, label, lconf, labels, label_div):
    """pvo_tsdf_panoptic_args of the label volumes label int32 / lconf f32 (both `shape`) and the frames' id maps labels int32
    [nframes,LH,LW]; None when none of the three is given (the plain call)"""
    if label is None and lconf is None and labels is None:
        return None
    if label is None or lconf is None or labels is None:
        raise PvoHipError("%s: label, lconf and labels come together" % what)
    for t, n in ((label, "label"), (lconf, "lconf"), (labels, "labels")):
        _contig(t, n)
        if t.device != dev:
            raise PvoHipError("%s: %s must be on %s" % (what, n, dev))
    if label.dtype != torch.int32 or lconf.dtype != torch.float32 or tuple(label.shape) != tuple(shape) or tuple(lconf.shape) != tuple(shape):
        raise PvoHipError("%s: label int32 and lconf f32 must have the shape of tsdf" % what)
    if labels.dtype != torch.int32 or labels.dim() < 3 or labels.shape[0] < nframes:
        raise PvoHipError("%s: labels must be int32 [nframes,LH,LW]" % what)
    p = _lib.TsdfPanopticArgs()
    p.label, p.lconf, p.labels = _ptr(label), _ptr(lconf), _ptr(labels)
    p.lh, p.lw, p.label_div = labels.shape[-2], labels.shape[-1], int(label_div)
    return p


def _mesh_labels(what, out, label, shape):
    """pvo_tsdf_mesh_labels_args for the label volume `label` (None: the plain call) and out["vlabel"] int32 [vcap]"""
    if label is None:
        return None
    _contig(label, "label")
    vlabel = out["vlabel"]
    if label.dtype != torch.int32 or tuple(label.shape) != tuple(shape) or label.device != out["verts"].device:
        raise PvoHipError("%s: label must be int32 with the shape of tsdf, on its device" % what)
    if vlabel.dtype != torch.int32 or vlabel.numel() < out["verts"].shape[0] or not vlabel.is_contiguous():
        raise PvoHipError("%s: out['vlabel'] must be int32 [vcap]" % what)
    p = _lib.TsdfMeshLabelsArgs()
    p.label, p.vlabel = _ptr(label), _ptr(vlabel)
    return p


def _check_dense(what, tsdf, wsum, rgb=None, with_rgb=True):
    """the shapes of a dense volume: tsdf / wsum [nz,ny,nx], rgb [nz,ny,nx,3] or None"""
    if tsdf.dim() != 3 or wsum.shape != tsdf.shape or (rgb is not None and tuple(rgb.shape) != tuple(tsdf.shape) + (3,)):
        raise PvoHipError("%s: tsdf and wsum must be [nz,ny,nx]%s" % (what, ", rgb [nz,ny,nx,3]" if with_rgb else ""))


def _fill_dense(a, tsdf, wsum, rgb, origin, voxel):
    """a dense volume and its placement into the fields every dense struct has (rgb: where the struct has one)"""
    a.tsdf, a.wsum = _ptr(tsdf), _ptr(wsum)
    if hasattr(a, "rgb"):
        a.rgb = _ptr(rgb)
    a.nz, a.ny, a.nx = tsdf.shape
    a.origin[0], a.origin[1], a.origin[2] = [float(v) for v in origin]
    a.voxel = float(voxel)


def _images(a, what, images, nframes, img_stride, img_offset, same_device_as=None):
    """the images block of a fusion: uint8 [nframes,3,IH,IW] BGR sampled at [img_offset::img_stride], or None"""
    if images is None:
        return
    _contig(images, "images")
    if same_device_as is not None:
        _dev(same_device_as, images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[0] < nframes or images.shape[1] != 3:
        raise PvoHipError("%s: images must be uint8 [nframes,3,IH,IW]" % what)
    a.images, a.IH, a.IW, a.img_stride, a.img_offset = _ptr(images), images.shape[2], images.shape[3], int(img_stride), int(img_offset)


def _kept(a, what, kept, dev):
    """the brick calls' optional survivor counts: int32 [cap] on the pool's device"""
    if kept is None:
        return
    _contig(kept, "kept")
    if kept.dtype != torch.int32 or kept.numel() < a.cap or kept.device != dev:
        raise PvoHipError("%s: kept must be an int32 device tensor of at least cap elements" % what)
    a.kept = _ptr(kept)


def _mesh_outputs(a, out):
    a.vcap, a.fcap = out["verts"].shape[0], out["faces"].shape[0]
    a.verts, a.normals, a.rgba, a.faces = _ptr(out["verts"]), _ptr(out.get("normals")), _ptr(out.get("rgba")), _ptr(out["faces"])
    a.counts = ctypes.c_void_p(out["counts"].data_ptr())


def _mesh(into, dev, vcap, fcap, labelled):
    """what tsdf_mesh and tsdf_sparse_mesh share: the buffers for vcap vertices and fcap faces, into(out), the counts read back - the
    call's one host synchronisation - and the same again with exactly the room needed if a capacity was exceeded"""
    while True:
        out = {"verts": torch.empty(vcap, 3, dtype=torch.float32, device=dev), "normals": torch.empty(vcap, 3, dtype=torch.float32, device=dev),
               "rgba": torch.empty(vcap, 4, dtype=torch.uint8, device=dev), "faces": torch.empty(fcap, 3, dtype=torch.int32, device=dev),
               "counts": torch.empty(2, dtype=torch.int32, device=dev)}
        if labelled:
            out["vlabel"] = torch.empty(vcap, dtype=torch.int32, device=dev)
        into(out)
        nv, nf = out["counts"].tolist()                 # the one synchronisation
        if nv <= vcap and nf <= fcap:
            break
        vcap, fcap = max(nv, vcap), max(nf, fcap)
    for k in ("verts", "normals", "rgba", "vlabel"):
        if k in out:
            out[k] = out[k][:nv]
    out["faces"] = out["faces"][:nf]
    return out


def tsdf_integrate(tsdf, wsum, rgb, poses, disps, intrinsics, ix, origin, voxel, trunc, weight=None, images=None, img_stride=8,
                   img_offset=3, z_near=0.0, w_max=0.0, label=None, lconf=None, labels=None, label_div=1):
    """Fuse keyframes ix, in that order, into the caller's volume in place (include/pvo_hip.h pvo_tsdf_integrate): tsdf / wsum f32
    [nz,ny,nx], rgb f32 [nz,ny,nx,3] or None (needs images); a zeroed volume is an empty one.  The centre of voxel (z,y,x) is
    origin + voxel * (x,y,z); poses [nframes,7] world-to-camera, disps [nframes,ht,wd] at any resolution with intrinsics [4] for it,
    weight f32 [nframes,ht,wd] or None (= 1), images uint8 [nframes,3,IH,IW] BGR sampled at [img_offset::img_stride], w_max 0 = no
    cap.  label int32 / lconf f32 [nz,ny,nx] with labels int32 [nframes,LH,LW] (ids read at (y // label_div, x // label_div), <= 0 =
    no segment) also fuse the segment ids (pvo_tsdf_integrate_panoptic); tsdf / wsum / rgb get the same bytes either way.
    No allocation beyond the cached workspace, no synchronisation."""
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb"), (poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"),
                 (ix, "ix"), (weight, "weight"), (images, "images")):
        if t is not None:
            _contig(t, n)
    dev = _dev(tsdf, wsum, rgb, poses, disps, intrinsics, ix, weight, images)
    _long(ix, "ix")
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb"), (poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"),
                 (weight, "weight")):
        if t is not None:
            _f32(t, n)
    _check_dense("tsdf_integrate", tsdf, wsum, rgb)
    N, (nf, ht, wd) = ix.shape[0], disps.shape
    if poses.shape[0] < nf or (weight is not None and weight.shape != disps.shape):
        raise PvoHipError("tsdf_integrate: poses must cover the frames of disps, weight must have the shape of disps")
    a = _lib.TsdfIntegrateArgs()
    _images(a, "tsdf_integrate", images, nf, img_stride, img_offset)
    _fill_dense(a, tsdf, wsum, rgb, origin, voxel)
    a.trunc, a.z_near, a.w_max = float(trunc), float(z_near), float(w_max)
    a.poses, a.disps, a.intrinsics, a.ix, a.weight = _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ix), _ptr(weight)
    a.N, a.nframes, a.ht, a.wd = N, nf, ht, wd
    p = _panoptic("tsdf_integrate", dev, tsdf.shape, nf, label, lconf, labels, label_div)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_integrate_workspace_bytes(N))
    with torch.cuda.device(dev):
        if p is None:
            check(lib.pvo_tsdf_integrate(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_integrate")
        else:
            check(lib.pvo_tsdf_integrate_panoptic(ctypes.byref(a), ctypes.byref(p), _ptr(ws), ws.numel(), _stream(dev)),
                  "tsdf_integrate_panoptic")


def tsdf_mesh_into(tsdf, wsum, rgb, origin, voxel, min_weight, out, label=None):
    """pvo_tsdf_mesh on caller-owned buffers (out: verts [vcap,3], faces [fcap,3], counts [2], optional normals / rgba).  Buffers keep
    whatever they held beyond the elements written.  label int32 [nz,ny,nx]: also one label per vertex into out["vlabel"] int32 [vcap]
    (pvo_tsdf_mesh_panoptic).  No allocation beyond the cached workspace, no synchronisation."""
    dev = tsdf.device
    a = _lib.TsdfMeshArgs()
    _fill_dense(a, tsdf, wsum, rgb, origin, voxel)
    a.min_weight = float(min_weight)
    _mesh_outputs(a, out)
    p = _mesh_labels("tsdf_mesh", out, label, tsdf.shape)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_mesh_workspace_bytes(a.nz, a.ny, a.nx))
    with torch.cuda.device(dev):
        if p is None:
            check(lib.pvo_tsdf_mesh(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_mesh")
        else:
            check(lib.pvo_tsdf_mesh_panoptic(ctypes.byref(a), ctypes.byref(p), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_mesh_panoptic")


def tsdf_mesh(tsdf, wsum, rgb, origin, voxel, min_weight=1.0, vcap=None, fcap=None, label=None):
    """The surface-nets mesh of a TSDF volume (include/pvo_hip.h pvo_tsdf_mesh).  Returns a dict: verts f32 [V,3], normals f32 [V,3],
    rgba uint8 [V,4] (rgb 0 without a colour volume), faces int32 [F,3], counts int32 [2] = (V, F), and with a label volume (int32
    [nz,ny,nx]) vlabel int32 [V].  Calls once with room for vcap
    vertices and fcap faces (default: a guess from the volume's faces), reads counts back - the call's one host synchronisation - and
    calls again with exactly the room needed if a capacity was exceeded."""
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb")):
        if t is not None:
            _contig(t, n)
            _f32(t, n)
    dev = _dev(tsdf, wsum, rgb)
    _check_dense("tsdf_mesh", tsdf, wsum, rgb)
    nz, ny, nx = tsdf.shape
    cells = max(nz - 1, 0) * max(ny - 1, 0) * max(nx - 1, 0)
    vcap = min(cells, 8 * (nz * ny + ny * nx + nz * nx)) if vcap is None else int(vcap)
    fcap = 2 * vcap if fcap is None else int(fcap)
    return _mesh(lambda out: tsdf_mesh_into(tsdf, wsum, rgb, origin, voxel, min_weight, out, label=label), dev, vcap, fcap, label is not None)


def _sparse_world(a, vol):
    """the brick volume's fields every sparse call shares, into those of them the struct `a` has.  vol: a dict (pvo_amd.tsdf_sparse.SparseTSDF.volume()) with grid int32
    [gz,gy,gx], coord int32 [cap,3], counts int32 [1], tsdf / wsum f32 [cap,8,8,8], rgb f32 [cap,8,8,8,3] or None, origin, voxel"""
    grid, coord, counts, tsdf, wsum, rgb = vol["grid"], vol["coord"], vol["counts"], vol["tsdf"], vol["wsum"], vol.get("rgb")
    for t, n in ((grid, "grid"), (coord, "coord"), (counts, "counts"), (tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb")):
        if t is not None:
            _contig(t, n)
    dev = _dev(grid, coord, counts, tsdf, wsum, rgb)
    B = _lib.TSDF_BRICK
    cap = tsdf.shape[0]
    if grid.dtype != torch.int32 or coord.dtype != torch.int32 or counts.dtype != torch.int32 or grid.dim() != 3 or counts.numel() < 1:
        raise PvoHipError("sparse tsdf: grid [gz,gy,gx], coord [cap,3] and counts [1] must be int32")
    if (tuple(tsdf.shape) != (cap, B, B, B) or wsum.shape != tsdf.shape or tuple(coord.shape) != (cap, 3)
            or (rgb is not None and tuple(rgb.shape) != (cap, B, B, B, 3))):
        raise PvoHipError("sparse tsdf: the pool must be tsdf / wsum [cap,8,8,8], rgb [cap,8,8,8,3], coord [cap,3]")
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb")):
        if t is not None:
            _f32(t, n)
    a.gz, a.gy, a.gx = grid.shape
    a.cap = cap
    a.origin[0], a.origin[1], a.origin[2] = [float(v) for v in vol["origin"]]
    a.voxel = float(vol["voxel"])
    if hasattr(a, "coord"):
        a.coord = _ptr(coord)
    if hasattr(a, "bricks"):
        a.bricks = _ptr(counts)
    return dev


def _sparse_frames(a, what, poses, disps, intrinsics, ix, weight):
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ix, "ix"), (weight, "weight")):
        if t is not None:
            _contig(t, n)
    _long(ix, "ix")
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (weight, "weight")):
        if t is not None:
            _f32(t, n)
    N, (nf, ht, wd) = ix.shape[0], disps.shape
    if poses.shape[0] < nf or (weight is not None and weight.shape != disps.shape):
        raise PvoHipError("%s: poses must cover the frames of disps, weight must have the shape of disps" % what)
    a.poses, a.disps, a.intrinsics, a.ix, a.weight = _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ix), _ptr(weight)
    a.N, a.nframes, a.ht, a.wd = N, nf, ht, wd


def tsdf_sparse_allocate(vol, poses, disps, intrinsics, ix, trunc, weight=None, z_near=0.0, margin=2.0):
    """Mark the bricks near the surfaces keyframes ix see and append the new ones to the pool of the brick volume `vol` (a dict, see
    _sparse_world; include/pvo_hip.h pvo_tsdf_sparse_allocate).  vol["counts"][0] becomes the number of bricks the volume wants, NOT
    clamped by the pool's capacity: the caller reads it and comes back with a larger pool (SparseTSDF.allocate does).  No allocation
    beyond the cached workspace, no synchronisation."""
    a = _lib.TsdfSparseAllocateArgs()
    dev = _sparse_world(a, vol)
    _dev(vol["grid"], poses, disps, intrinsics, ix, weight)
    _sparse_frames(a, "tsdf_sparse_allocate", poses, disps, intrinsics, ix, weight)
    a.grid = _ptr(vol["grid"])
    a.trunc, a.z_near, a.margin = float(trunc), float(z_near), float(margin)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_sparse_allocate_workspace_bytes(a.gz, a.gy, a.gx, a.N))
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_sparse_allocate(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_sparse_allocate")


def tsdf_sparse_integrate(vol, poses, disps, intrinsics, ix, trunc, weight=None, images=None, img_stride=8, img_offset=3, z_near=0.0,
                          w_max=0.0, kept=None, label=None, lconf=None, labels=None, label_div=1):
    """tsdf_integrate on the bricks in use of the brick volume `vol` (include/pvo_hip.h pvo_tsdf_sparse_integrate): every voxel of a
    brick gets the bytes the dense call leaves at that voxel; a frame is tested once per brick, not once per voxel.  kept: int32
    [cap] or None, per brick in use the number of slots of ix that survived the cull.  label int32 / lconf f32 [cap,8,8,8] with
    labels int32 [nframes,LH,LW] and label_div: the segment ids as well, as in tsdf_integrate (pvo_tsdf_sparse_integrate_panoptic).
    No allocation beyond the cached workspace, no synchronisation."""
    a = _lib.TsdfSparseIntegrateArgs()
    dev = _sparse_world(a, vol)
    _dev(vol["grid"], poses, disps, intrinsics, ix, weight, images)
    _sparse_frames(a, "tsdf_sparse_integrate", poses, disps, intrinsics, ix, weight)
    _images(a, "tsdf_sparse_integrate", images, a.nframes, img_stride, img_offset)
    a.tsdf, a.wsum, a.rgb = _ptr(vol["tsdf"]), _ptr(vol["wsum"]), _ptr(vol.get("rgb"))
    a.trunc, a.z_near, a.w_max = float(trunc), float(z_near), float(w_max)
    _kept(a, "tsdf_sparse_integrate", kept, dev)
    p = _panoptic("tsdf_sparse_integrate", dev, vol["tsdf"].shape, a.nframes, label, lconf, labels, label_div)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_sparse_integrate_workspace_bytes(a.N))
    with torch.cuda.device(dev):
        if p is None:
            check(lib.pvo_tsdf_sparse_integrate(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_sparse_integrate")
        else:
            check(lib.pvo_tsdf_sparse_integrate_panoptic(ctypes.byref(a), ctypes.byref(p), _ptr(ws), ws.numel(), _stream(dev)),
                  "tsdf_sparse_integrate_panoptic")


def _reintegrate_sets(a, what, dev, intrinsics, remove, add, images, img_stride, img_offset):
    """the two frame sets and the colour arguments of a re-integration into `a`; remove / add: (poses, disps, ix, weight or None) or
    None (no slot).  Returns (N_old, N)"""
    _contig(intrinsics, "intrinsics")
    _f32(intrinsics, "intrinsics")
    shape = None
    for s, (tag, sfx) in ((remove, ("remove", "_old")), (add, ("add", ""))):
        if s is None:
            continue
        poses, disps, ix, weight = s
        for t, n in ((poses, "poses"), (disps, "disps"), (ix, "ix"), (weight, "weight")):
            if t is not None:
                _contig(t, "%s %s" % (tag, n))
        _dev(intrinsics, poses, disps, ix, weight)
        _long(ix, "%s ix" % tag)
        for t, n in ((poses, "poses"), (disps, "disps"), (weight, "weight")):
            if t is not None:
                _f32(t, "%s %s" % (tag, n))
        if disps.dim() != 3 or poses.shape[0] < disps.shape[0] or (weight is not None and weight.shape != disps.shape):
            raise PvoHipError("%s: %s poses must cover the frames of disps [nframes,ht,wd], weight must have the shape of disps" % (what, tag))
        if shape is not None and tuple(disps.shape) != shape:
            raise PvoHipError("%s: the two sets must describe the same frames: disps %s against %s" % (what, tuple(disps.shape), shape))
        shape = tuple(disps.shape)
        setattr(a, "poses" + sfx, _ptr(poses))
        setattr(a, "disps" + sfx, _ptr(disps))
        setattr(a, "ix" + sfx, _ptr(ix))
        setattr(a, "weight" + sfx, _ptr(weight))
        setattr(a, "N" + sfx, ix.shape[0])
    a.intrinsics = _ptr(intrinsics)
    if shape is not None:
        a.nframes, a.ht, a.wd = shape
    _images(a, what, images, a.nframes, img_stride, img_offset, same_device_as=intrinsics)
    return a.N_old, a.N


def _reintegrate_workspace(what, dev, need, workspace):
    if workspace is None:
        return _workspace(dev, need)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != dev or workspace.numel() < need:
        raise PvoHipError("%s: workspace must be a contiguous uint8 device tensor of at least %d bytes" % (what, need))
    return workspace


def tsdf_reintegrate(tsdf, wsum, rgb, origin, voxel, trunc, intrinsics, remove=None, add=None, images=None, img_stride=8, img_offset=3,
                     z_near=0.0, w_max=0.0, w_floor=2.0 ** -10, workspace=None):
    """Take keyframes out of the caller's volume as they were fused and put keyframes in as they are now, in one pass (include/pvo_hip.h
    pvo_tsdf_reintegrate).  remove / add: (poses [nframes,7], disps [nframes,ht,wd], ix int64 [n], weight [nframes,ht,wd] or None) or
    None; `remove` holds the caller's SNAPSHOT of what was fused, `add` the present state; both over the same frames and one
    intrinsics [4].  Per voxel the remove slots run first, in order, then the add slots; a voxel whose weight falls to w_floor or
    below becomes empty (tsdf = wsum = rgb = 0).  images serves both sets.  A removal is approximate where w_max capped the weight.
    workspace: a caller-owned uint8 tensor of pvo_tsdf_reintegrate_workspace_bytes(n_remove, n_add), or None for the cached one.
    No allocation beyond that, no synchronisation."""
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb")):
        if t is not None:
            _contig(t, n)
            _f32(t, n)
    dev = _dev(tsdf, wsum, rgb, intrinsics)
    _check_dense("tsdf_reintegrate", tsdf, wsum, rgb)
    a = _lib.TsdfReintegrateArgs()
    n_old, n = _reintegrate_sets(a, "tsdf_reintegrate", dev, intrinsics, remove, add, images, img_stride, img_offset)
    _fill_dense(a, tsdf, wsum, rgb, origin, voxel)
    a.trunc, a.z_near, a.w_max, a.w_floor = float(trunc), float(z_near), float(w_max), float(w_floor)
    lib = _lib.load()
    ws = _reintegrate_workspace("tsdf_reintegrate", dev, lib.pvo_tsdf_reintegrate_workspace_bytes(n_old, n), workspace)
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_reintegrate(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_reintegrate")


def tsdf_sparse_reintegrate(vol, trunc, intrinsics, remove=None, add=None, images=None, img_stride=8, img_offset=3, z_near=0.0, w_max=0.0,
                            w_floor=2.0 ** -10, kept=None, workspace=None):
    """tsdf_reintegrate on the bricks in use of the brick volume `vol` (include/pvo_hip.h pvo_tsdf_sparse_reintegrate): every voxel of a
    brick gets the bytes the dense call leaves at that voxel.  Bricks for the poses of `add` must exist already
    (tsdf_sparse_allocate; SparseTSDF.reintegrate does it); bricks that become empty stay.  kept: int32 [cap] or None, survivors of
    the cull per brick, both sets summed."""
    a = _lib.TsdfSparseReintegrateArgs()
    dev = _sparse_world(a, vol)
    _dev(vol["grid"], intrinsics)
    n_old, n = _reintegrate_sets(a, "tsdf_sparse_reintegrate", dev, intrinsics, remove, add, images, img_stride, img_offset)
    a.tsdf, a.wsum, a.rgb = _ptr(vol["tsdf"]), _ptr(vol["wsum"]), _ptr(vol.get("rgb"))
    a.trunc, a.z_near, a.w_max, a.w_floor = float(trunc), float(z_near), float(w_max), float(w_floor)
    _kept(a, "tsdf_sparse_reintegrate", kept, dev)
    lib = _lib.load()
    ws = _reintegrate_workspace("tsdf_sparse_reintegrate", dev, lib.pvo_tsdf_sparse_reintegrate_workspace_bytes(n_old, n), workspace)
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_sparse_reintegrate(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_sparse_reintegrate")


def tsdf_sparse_mesh_into(vol, min_weight, out, label=None):
    """pvo_tsdf_sparse_mesh on caller-owned buffers (out as for tsdf_mesh_into; label int32 [cap,8,8,8]: out["vlabel"] as well,
    pvo_tsdf_sparse_mesh_panoptic).  No allocation beyond the cached workspace, no synchronisation."""
    a = _lib.TsdfSparseMeshArgs()
    dev = _sparse_world(a, vol)
    a.grid = _ptr(vol["grid"])
    a.tsdf, a.wsum, a.rgb = _ptr(vol["tsdf"]), _ptr(vol["wsum"]), _ptr(vol.get("rgb"))
    a.min_weight = float(min_weight)
    _mesh_outputs(a, out)
    p = _mesh_labels("tsdf_sparse_mesh", out, label, vol["tsdf"].shape)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_sparse_mesh_workspace_bytes(a.cap))
    with torch.cuda.device(dev):
        if p is None:
            check(lib.pvo_tsdf_sparse_mesh(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_sparse_mesh")
        else:
            check(lib.pvo_tsdf_sparse_mesh_panoptic(ctypes.byref(a), ctypes.byref(p), _ptr(ws), ws.numel(), _stream(dev)),
                  "tsdf_sparse_mesh_panoptic")


def tsdf_sparse_mesh(vol, min_weight=1.0, vcap=None, fcap=None, label=None):
    """The surface-nets mesh of a brick volume (include/pvo_hip.h pvo_tsdf_sparse_mesh), the dict of tsdf_mesh (vlabel with a label
    pool int32 [cap,8,8,8]); vertices in the order (slot, raster order inside the brick).  One host synchronisation (the counts), a second call if a capacity was exceeded."""
    dev = vol["tsdf"].device
    cap = vol["tsdf"].shape[0]
    vcap = min(cap * _lib.TSDF_BRICK ** 3, max(1024, 96 * cap)) if vcap is None else int(vcap)
    fcap = 2 * vcap if fcap is None else int(fcap)
    return _mesh(lambda out: tsdf_sparse_mesh_into(vol, min_weight, out, label=label), dev, vcap, fcap, label is not None)


RENDER_MAX_SAMPLES = 65536                 # (z_far - z_near) / dz of pvo_tsdf_render


def _render_range(what, dims, origin, voxel, poses, ix, dz, z_near, z_far):
    """(dz, z_near, z_far) with the defaults dz = voxel / 2 and z_far = the largest depth of a corner of the volume's box over the
    views ix (one small reduction read back: a synchronisation; none when z_far is given); raises where the range has more than
    RENDER_MAX_SAMPLES samples"""
    dz = 0.5 * float(voxel) if dz is None else float(dz)
    if z_far is None:
        nz, ny, nx = dims
        o = torch.tensor([float(v) for v in origin], dtype=torch.float64)
        ext = float(voxel) * torch.tensor([max(nx - 1, 0), max(ny - 1, 0), max(nz - 1, 0)], dtype=torch.float64)
        corners = torch.stack([o + ext * torch.tensor([(j >> 0) & 1, (j >> 1) & 1, (j >> 2) & 1], dtype=torch.float64) for j in range(8)])
        sel = ix[(ix >= 0) & (ix < poses.shape[0])]
        z_far = 0.0
        if sel.numel():
            p = poses[sel].double().cpu()
            x, y, z, w = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
            row = torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)         # the third row of R(q)
            z_far = float((row @ corners.T + p[:, 2:3]).max())
        z_far = max(z_far, float(z_near)) + dz
    z_near, z_far = float(z_near), float(z_far)
    if dz > 0 and (z_far - z_near) / dz > RENDER_MAX_SAMPLES:
        raise PvoHipError("%s: %g .. %g in steps of %g is more than %d samples per ray - raise dz (or bring z_near / z_far closer)"
                          % (what, z_near, z_far, dz, RENDER_MAX_SAMPLES))
    return dz, z_near, z_far


def _render_views(a, what, dev, poses, intrinsics, ix, ht, wd, label, normals, out):
    """the view and output fields both render calls share; returns the dict of outputs (caller-owned with out=)"""
    for t, n in ((poses, "poses"), (intrinsics, "intrinsics"), (ix, "ix")):
        _contig(t, n)
        if t.device != dev:
            raise PvoHipError("%s: %s must be on %s" % (what, n, dev))
    _long(ix, "ix")
    _f32(poses, "poses")
    _f32(intrinsics, "intrinsics")
    N, ht, wd = ix.shape[0], int(ht), int(wd)
    if poses.dim() != 2 or poses.shape[1] != 7 or intrinsics.numel() < 4:
        raise PvoHipError("%s: poses must be [nviews,7] and intrinsics [4]" % what)
    want = {"depth": ((N, ht, wd), torch.float32)}
    if normals:
        want["normal"] = ((N, ht, wd, 3), torch.float32)
    want["rgba"] = ((N, ht, wd, 4), torch.uint8)
    if label is not None:
        want["label"] = ((N, ht, wd), torch.int32)
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in want.items()}
    else:
        for k, t in out.items():
            known = dict(want, normal=((N, ht, wd, 3), torch.float32), visited=((N, ht, wd, 2), torch.int32))
            if k not in known or (k == "label" and label is None):
                raise PvoHipError("%s: out has no use for %r" % (what, k))
            shape, dt = known[k]
            if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise PvoHipError("%s: out[%r] must be a contiguous %s %s on %s" % (what, k, dt, list(shape), dev))
        if "depth" not in out:
            raise PvoHipError("%s: out needs 'depth'" % what)
    a.poses, a.intrinsics, a.ix = _ptr(poses), _ptr(intrinsics), _ptr(ix)
    a.N, a.nviews, a.ht, a.wd = N, poses.shape[0], ht, wd
    a.depth, a.normal, a.rgba = _ptr(out["depth"]), _ptr(out.get("normal")), _ptr(out.get("rgba"))
    a.out_label, a.visited = _ptr(out.get("label")), _ptr(out.get("visited"))
    return out


def tsdf_render(tsdf, wsum, rgb, origin, voxel, poses, intrinsics, ix, ht, wd, dz=None, z_near=0.0, z_far=None, min_weight=1.0, label=None,
                normals=True, out=None):
    """The volume seen from cameras (include/pvo_hip.h pvo_tsdf_render): per view ix[b] of poses [nviews,7] (world-to-camera) with
    intrinsics [4] for ht x wd pixels, the first zero crossing of the trilinear TSDF along every pixel's ray.  Returns a dict: depth f32
    [N,ht,wd] along the optical axis (0 = no surface), normal f32 [N,ht,wd,3] (world frame, outward; not with normals=False), rgba uint8
    [N,ht,wd,4] ((0,0,0,255) on hits without an rgb volume, 0 on misses) and, only with a label volume (int32 [nz,ny,nx]), label int32
    [N,ht,wd].  Rays are sampled at the depths k * dz between z_near and z_far.  Defaults: dz = 0.5 * voxel; z_far = the farthest
    corner of the volume's box over the views (plus one step), which reads the poses back once - pass z_far to stay asynchronous.  A
    range of more than 65536 samples raises: use a larger dz.  out=: caller-owned buffers (depth, and any of normal / rgba / label,
    visited int32 [N,ht,wd,2]) - with z_far given: no allocation beyond the cached workspace, no synchronisation, capturable."""
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb"), (label, "label")):
        if t is not None:
            _contig(t, n)
    dev = _dev(tsdf, wsum, rgb, label, poses, intrinsics, ix)
    for t, n in ((tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb")):
        if t is not None:
            _f32(t, n)
    _check_dense("tsdf_render", tsdf, wsum, rgb)
    if label is not None and (label.dtype != torch.int32 or label.shape != tsdf.shape):
        raise PvoHipError("tsdf_render: label must be int32 with the shape of tsdf")
    a = _lib.TsdfRenderArgs()
    out = _render_views(a, "tsdf_render", dev, poses, intrinsics, ix, ht, wd, label, normals, out)
    a.dz, a.z_near, a.z_far = _render_range("tsdf_render", tsdf.shape, origin, voxel, poses, ix, dz, z_near, z_far)
    _fill_dense(a, tsdf, wsum, rgb, origin, voxel)
    a.label, a.min_weight = _ptr(label), float(min_weight)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_render_workspace_bytes(a.N))
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_render(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_render")
    return out


def tsdf_sparse_render(vol, poses, intrinsics, ix, ht, wd, dz=None, z_near=0.0, z_far=None, min_weight=1.0, label=None, normals=True,
                       out=None):
    """tsdf_render of the brick volume `vol` (a dict, see _sparse_world; include/pvo_hip.h pvo_tsdf_sparse_render): the bytes of the dense
    render over the [8gz,8gy,8gx] volume that holds the bricks, with rays jumping over bricks that do not exist.  label: the label pool
    int32 [cap,8,8,8].  Defaults (dz = 0.5 * voxel, z_far from the world's box), out= and the sample limit as in tsdf_render."""
    a = _lib.TsdfSparseRenderArgs()
    dev = _sparse_world(a, vol)
    _dev(vol["grid"], poses, intrinsics, ix, label)
    if label is not None:
        _contig(label, "label")
        if label.dtype != torch.int32 or label.shape != vol["tsdf"].shape:
            raise PvoHipError("tsdf_sparse_render: label must be int32 with the shape of the pool")
    a.min_weight = float(min_weight)
    out = _render_views(a, "tsdf_sparse_render", dev, poses, intrinsics, ix, ht, wd, label, normals, out)
    B = _lib.TSDF_BRICK
    a.dz, a.z_near, a.z_far = _render_range("tsdf_sparse_render", (B * a.gz, B * a.gy, B * a.gx), vol["origin"], vol["voxel"], poses, ix,
                                            dz, z_near, z_far)
    a.grid, a.tsdf, a.wsum, a.rgb, a.label = _ptr(vol["grid"]), _ptr(vol["tsdf"]), _ptr(vol["wsum"]), _ptr(vol.get("rgb")), _ptr(label)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_sparse_render_workspace_bytes(a.N))
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_sparse_render(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_sparse_render")
    return out


def _track_frames(a, what, dev, poses, disps, intrinsics, ix, weight, iters, band, huber, lm, ep, min_count, system, residual, jac, out):
    """the frame, parameter and output fields both tracking calls share; returns the dict of outputs (caller-owned with out=)"""
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ix, "ix"), (weight, "weight")):
        if t is None:
            continue
        _contig(t, n)
        if t.device != dev:
            raise PvoHipError("%s: %s must be on %s" % (what, n, dev))
    _long(ix, "ix")
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (weight, "weight")):
        if t is not None:
            _f32(t, n)
    iters = int(iters)
    if not 0 <= iters <= _lib.TSDF_TRACK_MAX_ITERS:
        raise PvoHipError("%s: iters must lie in [0, %d]" % (what, _lib.TSDF_TRACK_MAX_ITERS))
    if disps.dim() != 3 or ix.dim() != 1 or tuple(poses.shape) != (ix.shape[0], 7) or intrinsics.numel() < 4:
        raise PvoHipError("%s: disps must be [nframes,ht,wd], ix [N], poses [N,7] (one start per slot) and intrinsics [4]" % what)
    if weight is not None and weight.shape != disps.shape:
        raise PvoHipError("%s: weight must have the shape of disps" % what)
    N, (nf, ht, wd) = ix.shape[0], disps.shape
    want = {"poses": ((N, 7), torch.float32), "info": ((N, iters + 1, 4), torch.float32)}
    optional = {"system": ((N, 27), torch.float64), "residual": ((N, ht, wd), torch.float32), "jac": ((N, ht, wd, 6), torch.float32)}
    for k, on in (("system", system), ("residual", residual), ("jac", jac)):
        if on:
            want[k] = optional[k]
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in want.items()}
    else:
        known = dict(want, **optional)
        for k, t in out.items():
            if k not in known:
                raise PvoHipError("%s: out has no use for %r" % (what, k))
            shape, dt = known[k]
            if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise PvoHipError("%s: out[%r] must be a contiguous %s %s on %s" % (what, k, dt, list(shape), dev))
        missing = [k for k in want if k not in out]
        if missing:
            raise PvoHipError("%s: out lacks %s (poses and info always, system / residual / jac when asked for)" % (what, ", ".join(missing)))
    a.poses, a.disps, a.intrinsics, a.ix, a.weight = _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ix), _ptr(weight)
    a.N, a.nframes, a.ht, a.wd = N, nf, ht, wd
    a.iters, a.min_count = iters, int(min_count)
    a.band, a.huber, a.lm, a.ep = float(band), float(huber), float(lm), float(ep)
    a.poses_out, a.info = _ptr(out["poses"]), _ptr(out["info"])
    a.system, a.residual, a.jac = _ptr(out.get("system")), _ptr(out.get("residual")), _ptr(out.get("jac"))
    return out


def tsdf_track(tsdf, wsum, origin, voxel, poses, disps, intrinsics, ix, weight=None, iters=10, band=0.9, huber=0.0, lm=1e-4, ep=1e-6,
               min_count=32, min_weight=1.0, system=False, residual=False, jac=False, out=None):
    """Frame-to-model tracking (include/pvo_hip.h pvo_tsdf_track): per slot s, the start pose poses[s] ([N,7], world-to-camera, ONE
    PER SLOT) refined by `iters` Gauss-Newton steps so that the back-projected pixels of frame ix[s] (disps [nframes,ht,wd] inverse
    depth, intrinsics [4] for ht x wd, weight like disps or None) lie on the zero level of the volume tsdf / wsum [nz,ny,nx].  Pixels
    with |S| < band (in truncations) vote; huber > 0 bounds a pixel's pull; lm, ep damp the 6 x 6 system; a slot with fewer than
    min_count voting pixels keeps its pose.  Returns a dict: poses f32 [N,7], info f32 [N,iters+1,4] = (E, count, max|xi| of the step
    taken, status) per evaluation (status 0 = stepped, 1 = too few pixels, 2 = factorisation failed, 4 = ix outside the frames), and on
    request system f64 [N,27] (the undamped H's upper triangle and b of the last evaluation), residual f32 [N,ht,wd] (S at the final
    pose, NaN where the pixel does not vote), jac f32 [N,ht,wd,6].
    The defaults band = 0.9, huber = 0 and min_count = 32 rest on nothing measured on real sequences: they are the values the
    analytic test scene was checked with.
    out=: caller-owned buffers (poses and info, and any of system / residual / jac: a buffer given is written whether or not its flag
    is set, a flag set without its buffer raises; out["poses"] may be `poses` itself) - then no
    allocation beyond the cached workspace, no synchronisation, capturable."""
    _contig(tsdf, "tsdf"); _contig(wsum, "wsum")
    dev = _dev(tsdf, wsum, poses, disps, intrinsics, ix, weight)
    _f32(tsdf, "tsdf"); _f32(wsum, "wsum")
    _check_dense("tsdf_track", tsdf, wsum, with_rgb=False)
    a = _lib.TsdfTrackArgs()
    out = _track_frames(a, "tsdf_track", dev, poses, disps, intrinsics, ix, weight, iters, band, huber, lm, ep, min_count, system, residual,
                        jac, out)
    _fill_dense(a, tsdf, wsum, None, origin, voxel)
    a.min_weight = float(min_weight)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_track_workspace_bytes(a.N, a.ht, a.wd))
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_track(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_track")
    return out


def tsdf_sparse_track(vol, poses, disps, intrinsics, ix, weight=None, iters=10, band=0.9, huber=0.0, lm=1e-4, ep=1e-6, min_count=32,
                      min_weight=1.0, system=False, residual=False, jac=False, out=None):
    """tsdf_track against the brick volume `vol` (a dict, see _sparse_world; include/pvo_hip.h pvo_tsdf_sparse_track): every output has
    the bytes of tsdf_track over the [8gz,8gy,8gx] volume that holds the bricks.  Parameters, defaults (which rest on nothing measured
    on real sequences), outputs and out= as in tsdf_track."""
    a = _lib.TsdfSparseTrackArgs()
    dev = _sparse_world(a, vol)
    _dev(vol["grid"], poses, disps, intrinsics, ix, weight)
    a.min_weight = float(min_weight)
    out = _track_frames(a, "tsdf_sparse_track", dev, poses, disps, intrinsics, ix, weight, iters, band, huber, lm, ep, min_count, system,
                        residual, jac, out)
    a.grid, a.tsdf, a.wsum = _ptr(vol["grid"]), _ptr(vol["tsdf"]), _ptr(vol["wsum"])
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_tsdf_sparse_track_workspace_bytes(a.N, a.ht, a.wd))
    with torch.cuda.device(dev):
        check(lib.pvo_tsdf_sparse_track(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "tsdf_sparse_track")
    return out


def object_motion(poses, disps, intrinsics, labels, ii, jj, target, job_edge, job_label, weight=None, start=None, iters=8, z_min=0.25,
                  huber=0.0, lm=1e-4, ep=1e-6, min_count=16, system=False, centroid=False, residual=False, jac=False, out=None):
    """Per-instance rigid motion from point correspondences (include/pvo_hip.h pvo_object_motion): per job n - the edge job_edge[n]
    (int64 [N], into ii / jj int64 [E]) and the label job_label[n] (int32 [N]) - the A in SE(3) that takes the points of frame
    i = ii[e] with that label (labels int32 [nframes,ht,wd], disps [nframes,ht,wd] inverse depth, intrinsics [4] for ht x wd) from
    camera i at time i to camera j at time j, so that they project onto target [E,ht,wd,2] (ABSOLUTE pixel coordinates in frame j, the
    object's motion included: the factor graph's coords0 + full_flow), weighted by weight [E,ht,wd] or None.  `iters` Gauss-Newton
    steps from start [N,7] (None: G_j G_i^-1 of poses [nframes,7], the object at rest); pixels with depth beyond z_min in camera j
    contribute; huber > 0 bounds a pixel's pull (in pixels); lm, ep damp the 6 x 6 system; a job with fewer than min_count
    contributing pixels keeps its A.  Returns a dict: rel f32 [N,7] (the final A), motion f32 [N,7] (G_j^-1 A G_i, the motion in the
    world frame: the identity for a static segment), info f32 [N,iters+1,4] = (E, count, max|xi| of the step taken, status) per
    evaluation (status 0 = stepped, 1 = too few pixels, 2 = factorisation failed, 4 = no such edge or frame), and on request system
    f64 [N,27] (the undamped H's upper triangle and b of the last evaluation), centroid f32 [N,3] (the contributing points' mean in
    the world at time i), residual f32 [N,ht,wd,2] (NaN where the pixel does not contribute) and jac f32 [N,ht,wd,2,6].
    The defaults iters = 8, z_min = 0.25, huber = 0, lm = 1e-4, ep = 1e-6 and min_count = 16 rest on nothing measured on real
    sequences: they are the values the analytic test scene was checked with.
    Shapes, dtypes, devices and contiguity are checked here (ValueError).
    out=: caller-owned buffers (rel, motion and info, and any of system / centroid / residual / jac: a buffer given is written whether
    or not its flag is set, a flag set without its buffer raises; out["rel"] may be `start` itself) - then no allocation beyond the
    cached workspace, no synchronisation, capturable."""
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    named = (("poses", poses, f32), ("disps", disps, f32), ("intrinsics", intrinsics, f32), ("labels", labels, i32), ("ii", ii, i64),
             ("jj", jj, i64), ("target", target, f32), ("job_edge", job_edge, i64), ("job_label", job_label, i32),
             ("weight", weight, f32), ("start", start, f32))
    dev = None
    for name, t, dt in named:
        if t is None:
            if name in ("weight", "start"):
                continue
            raise ValueError("object_motion: %s is required" % name)
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("object_motion: %s must be a device tensor (there is no CPU fallback)" % name)
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError("object_motion: %s must be on %s" % (name, dev))
        if t.dtype != dt:
            raise ValueError("object_motion: %s must be %s" % (name, dt))
        if not t.is_contiguous():
            raise ValueError("object_motion: %s must be contiguous" % name)
    if disps.dim() != 3 or labels.shape != disps.shape or poses.shape != (disps.shape[0], 7) or intrinsics.numel() < 4:
        raise ValueError("object_motion: disps and labels must be [nframes,ht,wd], poses [nframes,7] and intrinsics [4]")
    nf, ht, wd = disps.shape
    if ii.dim() != 1 or jj.shape != ii.shape or tuple(target.shape) != (ii.shape[0], ht, wd, 2):
        raise ValueError("object_motion: ii and jj must be [E] and target [E,ht,wd,2]")
    E = ii.shape[0]
    if weight is not None and tuple(weight.shape) != (E, ht, wd):
        raise ValueError("object_motion: weight must be [E,ht,wd]")
    if job_edge.dim() != 1 or job_label.shape != job_edge.shape:
        raise ValueError("object_motion: job_edge and job_label must be [N]")
    N = job_edge.shape[0]
    if start is not None and tuple(start.shape) != (N, 7):
        raise ValueError("object_motion: start must be [N,7] (one per job)")
    iters = int(iters)
    if not 0 <= iters <= _lib.OBJECT_MOTION_MAX_ITERS:
        raise ValueError("object_motion: iters must lie in [0, %d]" % _lib.OBJECT_MOTION_MAX_ITERS)
    want = {"rel": ((N, 7), f32), "motion": ((N, 7), f32), "info": ((N, iters + 1, 4), f32)}
    optional = {"system": ((N, 27), torch.float64), "centroid": ((N, 3), f32), "residual": ((N, ht, wd, 2), f32),
                "jac": ((N, ht, wd, 2, 6), f32)}
    for k, on in (("system", system), ("centroid", centroid), ("residual", residual), ("jac", jac)):
        if on:
            want[k] = optional[k]
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in want.items()}
    else:
        known = dict(want, **optional)
        for k, t in out.items():
            if k not in known:
                raise ValueError("object_motion: out has no use for %r" % (k,))
            shape, dt = known[k]
            if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError("object_motion: out[%r] must be a contiguous %s %s on %s" % (k, dt, list(shape), dev))
        missing = [k for k in want if k not in out]
        if missing:
            raise ValueError("object_motion: out lacks %s (rel, motion and info always, the others when asked for)" % ", ".join(missing))
    a = _lib.ObjectMotionArgs()
    a.poses, a.disps, a.intrinsics, a.labels = _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(labels)
    a.ii, a.jj, a.target, a.weight = _ptr(ii), _ptr(jj), _ptr(target), _ptr(weight)
    a.job_edge, a.job_label, a.start = _ptr(job_edge), _ptr(job_label), _ptr(start)
    a.N, a.E, a.nframes, a.ht, a.wd = N, E, nf, ht, wd
    a.iters, a.min_count = iters, int(min_count)
    a.z_min, a.huber, a.lm, a.ep = float(z_min), float(huber), float(lm), float(ep)
    a.rel, a.motion, a.info = _ptr(out["rel"]), _ptr(out["motion"]), _ptr(out["info"])
    a.system, a.centroid, a.residual, a.jac = _ptr(out.get("system")), _ptr(out.get("centroid")), _ptr(out.get("residual")), _ptr(out.get("jac"))
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_object_motion_workspace_bytes(N, ht, wd))
    with torch.cuda.device(dev):
        check(lib.pvo_object_motion(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "object_motion")
    return out


def segment_associate(labels, ii, jj, target, S, valid=None, cls=None, min_iou=0.25, out=None, form=0):
    """Segments associated across keyframes (include/pvo_hip.h pvo_segment_associate): per edge e the segments of frame ii[e] (labels
    int32 [nframes,ht,wd], dense in [0, S), 0 = no segment) carried to target [E,ht,wd,2] (ABSOLUTE (x, y) in frame jj[e]: the factor
    graph's coords0 + full_flow, rounded to the nearest pixel; a pixel that leaves the frame or is not finite is dropped), counted
    against frame jj[e]'s labels and matched by mutual best IoU.  valid uint8 [E,ht,wd] or None: only nonzero pixels count; cls int32
    [nframes,S] or None: segments of different class never match; min_iou: the least IoU of a match.  ii, jj int64 [E].
    Returns a dict of int32 tensors: overlap [E,S,S], area_i [E,S] (counted pixels per source label), area_j [E,S] (frame jj[e]'s
    pixels per label), match [E,S] (the label of frame jj[e] matched to a, or -1), match_n, match_d [E,S] (the matched pair's IoU as
    the fraction n / d; 0 without a match).  Integers throughout: the same operands give the same bytes.
    Shapes, dtypes, devices and contiguity are checked here (ValueError).  out=: caller-owned buffers for all six - then no allocation,
    no synchronisation, capturable.  form=1 (S <= 128): the counting kernel keeps its table in LDS (measurements; the same bytes)."""
    i32, i64 = torch.int32, torch.int64
    named = (("labels", labels, i32), ("ii", ii, i64), ("jj", jj, i64), ("target", target, torch.float32), ("valid", valid, torch.uint8),
             ("cls", cls, i32))
    dev = None
    for name, t, dt in named:
        if t is None:
            if name in ("valid", "cls"):
                continue
            raise ValueError("segment_associate: %s is required" % name)
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("segment_associate: %s must be a device tensor (there is no CPU fallback)" % name)
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError("segment_associate: %s must be on %s" % (name, dev))
        if t.dtype != dt:
            raise ValueError("segment_associate: %s must be %s" % (name, dt))
        if not t.is_contiguous():
            raise ValueError("segment_associate: %s must be contiguous" % name)
    if labels.dim() != 3:
        raise ValueError("segment_associate: labels must be [nframes,ht,wd]")
    nf, ht, wd = labels.shape
    if ht * wd >= 1 << 24:
        raise ValueError("segment_associate: ht * wd must stay below 2^24 (the IoU threshold is exact up to there)")
    if ii.dim() != 1 or jj.shape != ii.shape or tuple(target.shape) != (ii.shape[0], ht, wd, 2):
        raise ValueError("segment_associate: ii and jj must be [E] and target [E,ht,wd,2]")
    E, S = ii.shape[0], int(S)
    if not 1 <= S <= _lib.SEGMENT_ASSOC_MAX_S:
        raise ValueError("segment_associate: S must lie in [1, %d]" % _lib.SEGMENT_ASSOC_MAX_S)
    if valid is not None and tuple(valid.shape) != (E, ht, wd):
        raise ValueError("segment_associate: valid must be [E,ht,wd]")
    if cls is not None and tuple(cls.shape) != (nf, S):
        raise ValueError("segment_associate: cls must be [nframes,S]")
    min_iou = float(min_iou)
    if not (min_iou >= 0.0 and min_iou != float("inf")):
        raise ValueError("segment_associate: min_iou must be finite and >= 0")
    want = {"overlap": (E, S, S), "area_i": (E, S), "area_j": (E, S), "match": (E, S), "match_n": (E, S), "match_d": (E, S)}
    if out is None:
        out = {k: torch.empty(shape, dtype=i32, device=dev) for k, shape in want.items()}
    else:
        if set(out) != set(want):
            raise ValueError("segment_associate: out must hold exactly %s" % ", ".join(want))
        for k, shape in want.items():
            t = out[k]
            if not torch.is_tensor(t) or t.dtype != i32 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError("segment_associate: out[%r] must be a contiguous int32 %s on %s" % (k, list(shape), dev))
    a = _lib.SegmentAssocArgs()
    a.labels, a.ii, a.jj, a.target, a.valid, a.cls = _ptr(labels), _ptr(ii), _ptr(jj), _ptr(target), _ptr(valid), _ptr(cls)
    a.E, a.nframes, a.ht, a.wd, a.S, a.min_iou, a.form = E, nf, ht, wd, S, min_iou, int(form)
    a.overlap, a.area_i, a.area_j = _ptr(out["overlap"]), _ptr(out["area_i"]), _ptr(out["area_j"])
    a.match, a.match_n, a.match_d = _ptr(out["match"]), _ptr(out["match_n"]), _ptr(out["match_d"])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_segment_associate(ctypes.byref(a), _stream(dev)), "segment_associate")
    return out


_TRANSPORT_MODES = {"nearest": _lib.TRANSPORT_NEAREST, "reference": _lib.TRANSPORT_REFERENCE}


def feature_transport(ref_feats, cur_feats, flow, scales=None, depth=None, order=1, rel_pose=None, intrinsics=None, alpha=1.0,
                      mode="nearest", out=None):
    """The previous frame's feature pyramid carried along the flow into the current frame (include/pvo_hip.h pvo_feature_transport):
    a forward splat, the depth key deciding between the cells that land on one target.  ref_feats: a list of up to 8 channels-last
    [1,C,H,W] tensors (float16, bfloat16 or float32, one C and dtype, C * itemsize % 16 == 0); cur_feats: the same shapes, or None.
    flow float32 [Hf,Wf,2] (x, y); scales: per level (sx, sy), level cells per flow unit (nearest mode; None = 1); depth float32 [Hd,Wd]
    or None; order +1: the smallest key wins (a depth), -1: the largest (a disparity); rel_pose 12 float32 ([R|t] rows, reference
    camera -> current camera) with intrinsics float32 [4] at the depth map's resolution: the depth is carried into the current camera
    first (order +1 only).  mode "nearest" (flow scaled to the level, rounded to nearest) or "reference" (the reference's rules).
    Returns (outs, srcs): outs[l] channels-last [1,2C,H,W] = [cur | alpha * transported] ([1,C,H,W] without cur_feats), srcs[l] int32
    [H,W], the source cell that won each cell or -1.  Shapes, dtypes, devices and contiguity are checked here (ValueError).
    out=(outs, srcs): caller-owned buffers - then no allocation, no synchronisation, capturable."""
    f32 = torch.float32
    if not isinstance(ref_feats, (list, tuple)) or len(ref_feats) > _lib.TRANSPORT_MAX_LEVELS:
        raise ValueError("feature_transport: ref_feats must be a list of at most %d tensors" % _lib.TRANSPORT_MAX_LEVELS)
    L = len(ref_feats)
    if cur_feats is not None and (not isinstance(cur_feats, (list, tuple)) or len(cur_feats) != L):
        raise ValueError("feature_transport: cur_feats must be None or a list as long as ref_feats")
    if mode not in _TRANSPORT_MODES:
        raise ValueError("feature_transport: mode must be 'nearest' or 'reference'")
    if order not in (1, -1):
        raise ValueError("feature_transport: order must be +1 (smallest key wins) or -1 (largest key wins)")
    alpha = float(alpha)
    if alpha != alpha or alpha in (float("inf"), float("-inf")):
        raise ValueError("feature_transport: alpha must be finite")
    if rel_pose is not None and (depth is None or intrinsics is None):
        raise ValueError("feature_transport: rel_pose needs depth and intrinsics")
    if rel_pose is not None and order != 1:
        raise ValueError("feature_transport: rel_pose carries a depth, not a disparity (order must be +1)")
    if rel_pose is None and intrinsics is not None:
        raise ValueError("feature_transport: intrinsics are given only with rel_pose")
    dev = None
    for name, t, shape in (("flow", flow, (None, None, 2)), ("depth", depth, (None, None)), ("rel_pose", rel_pose, None),
                           ("intrinsics", intrinsics, (4,))):
        if t is None:
            if name == "flow":
                raise ValueError("feature_transport: flow is required")
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("feature_transport: %s must be a device tensor (there is no CPU fallback)" % name)
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError("feature_transport: %s must be on %s" % (name, dev))
        if t.dtype != f32 or not t.is_contiguous():
            raise ValueError("feature_transport: %s must be contiguous float32" % name)
        if shape is None:
            if t.numel() != 12:
                raise ValueError("feature_transport: rel_pose must hold 12 values, the rows of [R|t]")
        elif t.dim() != len(shape) or any(w is not None and w != n for w, n in zip(shape, t.shape)):
            raise ValueError("feature_transport: %s must be %s" % (name, {"flow": "[Hf,Wf,2]", "depth": "[Hd,Wd]", "intrinsics": "[4]"}[name]))
    C = dtype = None
    for l in range(L):
        for name, t in (("ref_feats", ref_feats[l]), ("cur_feats", None if cur_feats is None else cur_feats[l])):
            if t is None:
                if name == "ref_feats":
                    raise ValueError("feature_transport: ref_feats[%d] is required" % l)
                continue
            if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
                raise ValueError("feature_transport: %s[%d] must be a tensor on %s (there is no CPU fallback)" % (name, l, dev))
            if t.dim() != 4 or t.shape[0] != 1 or not t.is_contiguous(memory_format=torch.channels_last):
                raise ValueError("feature_transport: %s[%d] must be a channels-last [1,C,H,W] tensor" % (name, l))
            if C is None:
                C, dtype = t.shape[1], t.dtype
                if dtype not in (torch.float16, torch.bfloat16, f32) or C < 1 or (C * t.element_size()) % 16:
                    raise ValueError("feature_transport: features must be float16, bfloat16 or float32 with C * itemsize % 16 == 0")
            if t.shape[1] != C or t.dtype != dtype:
                raise ValueError("feature_transport: every level must have the same C and dtype")
            if name == "cur_feats" and t.shape != ref_feats[l].shape:
                raise ValueError("feature_transport: cur_feats[%d] must have ref_feats[%d]'s shape" % (l, l))
        if ref_feats[l].shape[2] * ref_feats[l].shape[3] >= 1 << 31:
            raise ValueError("feature_transport: H * W must stay below 2^31")
    if L and (flow.shape[0] < 1 or flow.shape[1] < 1 or (depth is not None and depth.numel() == 0)):
        raise ValueError("feature_transport: flow and depth must not be empty")
    if scales is None:
        scales = [(1.0, 1.0)] * L
    if len(scales) != L or any(len(s) != 2 for s in scales):
        raise ValueError("feature_transport: scales must give (sx, sy) per level")
    shapes = [tuple(t.shape[2:]) for t in ref_feats]
    widths = [C * (1 if cur_feats is None or cur_feats[l] is None else 2) for l in range(L)]
    if out is None:
        outs = [_new_cl(1, widths[l], shapes[l][0], shapes[l][1], dtype, dev) for l in range(L)]
        srcs = [torch.empty(shapes[l], dtype=torch.int32, device=dev) for l in range(L)]
    else:
        outs, srcs = out
        if len(outs) != L or len(srcs) != L:
            raise ValueError("feature_transport: out must be (outs, srcs), one tensor per level each")
        for l in range(L):
            o, s = outs[l], srcs[l]
            if not torch.is_tensor(o) or o.device != dev or o.dtype != dtype or tuple(o.shape) != (1, widths[l]) + shapes[l] or \
                    not o.is_contiguous(memory_format=torch.channels_last):
                raise ValueError("feature_transport: outs[%d] must be a channels-last %s [1,%d,%d,%d] on %s"
                                 % (l, dtype, widths[l], shapes[l][0], shapes[l][1], dev))
            if not torch.is_tensor(s) or s.device != dev or s.dtype != torch.int32 or tuple(s.shape) != shapes[l] or not s.is_contiguous():
                raise ValueError("feature_transport: srcs[%d] must be a contiguous int32 %s on %s" % (l, list(shapes[l]), dev))
    if L == 0:
        return list(outs), list(srcs)
    a = _lib.FeatureTransportArgs()
    a.flow, a.Hf, a.Wf = _ptr(flow), flow.shape[0], flow.shape[1]
    a.depth, a.rel_pose, a.intrinsics = _ptr(depth), _ptr(rel_pose), _ptr(intrinsics)
    a.Hd, a.Wd = (0, 0) if depth is None else depth.shape
    a.C, a.dtype, a.L, a.mode, a.order, a.alpha = C, _DT[dtype], L, _TRANSPORT_MODES[mode], order, alpha
    for l in range(L):
        v = a.level[l]
        v.ref, v.out, v.src = _ptr(ref_feats[l]), _ptr(outs[l]), _ptr(srcs[l])
        v.cur = _ptr(None if cur_feats is None else cur_feats[l])
        v.H, v.W = shapes[l]
        v.sx, v.sy = float(scales[l][0]), float(scales[l][1])
    lib = _lib.load()
    need = lib.pvo_feature_transport_workspace_bytes(ctypes.byref(a))
    ws = _workspace(dev, need)
    with torch.cuda.device(dev):
        check(lib.pvo_feature_transport(ctypes.byref(a), _ptr(ws), ws.numel(), _stream(dev)), "feature_transport")
    return list(outs), list(srcs)


def _baseline(baseline, what):
    """a stereo baseline: a finite number >= 0 (0 = no stereo edges)"""
    b = float(baseline)
    if not (0.0 <= b < float("inf")):
        raise PvoHipError("%s: the stereo baseline must be finite and >= 0, got %r" % (what, baseline))
    return b


def reproject(poses, disps, intrinsics, ii, jj, out=None, baseline=0.0):
    """DepthVideo.reproject (depth_video.py:154-163): poses [F,7], disps [F,ht,wd],
    intrinsics [F,4] -> coords [E,ht,wd,2], valid [E,ht,wd,1].  out: a contiguous fp32 [E,ht,wd,2] tensor to write the
    coordinates into (e.g. the rows of a state buffer).  baseline > 0 (pvo_reproject_rig): an edge (i, i) is a stereo edge,
    u_right = u - fx b d; 0 is pvo_reproject."""
    baseline = _baseline(baseline, "reproject")
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj")):
        _contig(t, n)
    dev = _dev(poses, disps, intrinsics, ii, jj)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics"); _long(ii, "ii"); _long(jj, "jj")
    E, ht, wd = ii.shape[0], disps.shape[1], disps.shape[2]
    if out is not None:
        if tuple(out.shape) != (E, ht, wd, 2) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("reproject: out must be a contiguous float32 [E,ht,wd,2] tensor on the inputs' device")
        coords = out
    else:
        coords = torch.empty(E, ht, wd, 2, dtype=torch.float32, device=dev)
    valid = torch.empty(E, ht, wd, 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if baseline == 0.0:
            check(_lib.load().pvo_reproject(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj),
                                            _ptr(coords), _ptr(valid), E, ht, wd, _stream(dev)), "reproject")
        else:
            check(_lib.load().pvo_reproject_rig(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj),
                                                _ptr(coords), _ptr(valid), E, ht, wd, baseline, _stream(dev)), "reproject (stereo)")
    return coords, valid


def edge_rows_init(nets, poses, disps, intrinsics, ii, jj, net, target, weight, raw_mask, delta_dy, baseline=0.0):
    """pvo_edge_rows_init: the state rows of n new edges in one launch - net[e] = nets[ii[e]], target[e] = the reprojection of
    edge e (reproject's coordinates, bit for bit), zero weight / raw_mask / delta_dy.  nets [F,ht,wd,128] 16-bit frame rows,
    net [n,ht,wd,128] in the same dtype, the four f32 tensors [n,ht,wd,2]: contiguous (the new rows of the caller's buffers)."""
    baseline = _baseline(baseline, "edge_rows_init")
    dev = _dev(nets, poses, disps, intrinsics, ii, jj, net, target, weight, raw_mask, delta_dy)
    _f32(poses, "poses"); _f32(disps, "disps"); _f32(intrinsics, "intrinsics"); _long(ii, "ii"); _long(jj, "jj")
    n, ht, wd = ii.shape[0], disps.shape[1], disps.shape[2]
    for t, name in ((nets, "nets"), (poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj"), (net, "net")):
        _contig(t, name)
    if nets.dtype not in (torch.float16, torch.bfloat16) or net.dtype != nets.dtype or tuple(nets.shape[1:]) != (ht, wd, 128) or \
            tuple(net.shape) != (n, ht, wd, 128) or jj.shape[0] != n or nets.shape[0] != disps.shape[0]:
        raise PvoHipError("edge_rows_init: nets [F,ht,wd,128] and net [n,ht,wd,128] must be 16-bit tensors of one dtype")
    for t, name in ((target, "target"), (weight, "weight"), (raw_mask, "raw_mask"), (delta_dy, "delta_dy")):
        if tuple(t.shape) != (n, ht, wd, 2) or t.dtype != torch.float32 or not t.is_contiguous():
            raise PvoHipError("edge_rows_init: %s must be a contiguous float32 [n,ht,wd,2] tensor" % name)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_edge_rows_init(_ptr(nets), _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj), _ptr(net),
                                             _ptr(target), _ptr(weight), _ptr(raw_mask), _ptr(delta_dy), n, ht, wd, baseline,
                                             _stream(dev)), "edge_rows_init")


# --------------------------------------------------------------------------- bundle adjustment
def _sens_map(disps_sens, disps, what):
    """the sensor map of a depth BA: fp32, contiguous, disps' shape and device"""
    _f32(disps_sens, "disps_sens")
    _contig(disps_sens, "disps_sens")
    if tuple(disps_sens.shape) != tuple(disps.shape) or disps_sens.device != disps.device:
        raise PvoHipError("%s: disps_sens must have disps' shape %s and device" % (what, tuple(disps.shape)))


def _ba_operands(what, poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, *more_device, eta_f32=True, window_from_zero=True):
    """the operand checks `ba`, `ba_uncertainty` and `ba_calib` share: contiguity, one device, dtypes, the pose window ->
    (dev, F, ht, wd, HW, E, t0, t1, P).  `ba` switches two of them off: eta_f32 (its eta may be None, and it checks the dtype
    itself) and window_from_zero (it leaves a negative or reversed window to the library)."""
    for t, n in ((targets, "targets"), (weights, "weights"), (poses, "poses"), (disps, "disps"),
                 (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj")):
        _contig(t, n)      # droid.cpp:103-109 checks exactly these
    dev = _dev(poses, disps, intrinsics, targets, weights, eta, ii, jj, *more_device)
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (targets, "targets"),
                 (weights, "weights")) + (((eta, "eta"),) if eta_f32 else ()):
        _f32(t, n)
    _long(ii, "ii"); _long(jj, "jj")
    F, ht, wd = disps.shape
    t0, t1 = int(t0), int(t1)
    P = t1 - t0
    if (window_from_zero and (P < 0 or t0 < 0)) or poses.shape[0] < t1 or F < t1:
        raise PvoHipError("%s: pose window [%d,%d) exceeds the buffers (%d poses, %d depth maps)"
                          % (what, t0, t1, poses.shape[0], F))
    return dev, F, ht, wd, ht * wd, ii.shape[0], t0, t1, P


def _depth_rows(K_eta, t0, t1, ii, dev):
    """K = |unique([t0,t1) U ii)|, the rows of dz, is only known on the device.  eta carries one row per depth map (the
    reference's C + eta broadcast requires it), so K == K_eta unless eta is a single broadcast row; only then is K read back
    (one sync)."""
    return K_eta if K_eta > 1 else int(torch.unique(torch.cat([torch.arange(t0, t1, device=dev), ii])).numel())


def _status4(status, what):
    if status is not None and (status.dtype != torch.int32 or status.numel() < 4):
        raise PvoHipError("%s: status must be int32 with 4 elements" % what)


def ba(poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, motion_only,
       status=None, disps_sens=None, alpha=0.05, stereo_baseline=0.0):
    """droid.cpp:87-114 / ba_cuda droid_kernels.cu:1293-1410.

    poses [F,7] and disps [F,ht,wd] are updated IN PLACE; returns [dx [P,6], dz [K,ht*wd]]
    (dz is an empty tensor when motion_only, where the reference returns an undefined one).
    Fully asynchronous: no host synchronisation.  `status` (optional int32[4] device tensor)
    receives [non-SPD seen, K, eta-row mismatch, 0].
    disps_sens [F,ht,wd] (optional): measured inverse depth, 0 = no measurement - the sensor-depth prior with weight
    `alpha` (pvo_ba_prior, include/pvo_hip.h); None is pvo_ba.
    stereo_baseline > 0 (pvo_ba_rig): an edge (i, i) is a stereo edge of a rectified rig with that baseline; 0 changes nothing."""
    stereo_baseline = _baseline(stereo_baseline, "ba")
    if disps_sens is not None:
        _sens_map(disps_sens, disps, "ba")
    dev, F, ht, wd, HW, E, t0, t1, P = _ba_operands("ba", poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1,
                                                    eta_f32=False, window_from_zero=False)
    if eta is not None and not motion_only:
        _f32(eta, "eta")
        eta = eta.contiguous().view(-1, HW)     # droid_kernels.cu:1376 eta.view({-1, ht*wd})
        K_eta = eta.shape[0]
    else:
        K_eta = 1
        if not motion_only:
            raise PvoHipError("ba: eta is required unless motion_only")
    K = 0 if motion_only or E + P == 0 else _depth_rows(K_eta, t0, t1, ii, dev)
    dx = torch.zeros(max(P, 0), 6, dtype=torch.float32, device=dev)
    dz = torch.zeros(K, HW, dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = lib.pvo_ba_workspace_bytes(E, P, F, HW)
    ws = _workspace(dev, nbytes)
    with torch.cuda.device(dev):
        args = (_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(targets), _ptr(weights),
                _vp(eta), _ptr(ii), _ptr(jj),
                E, F, ht, wd, K_eta, t0, t1, int(iterations), float(lm), float(ep),
                1 if motion_only else 0, _ptr(dx), _ptr(dz), K, _vp(status),
                ctypes.c_void_p(ws.data_ptr()), ws.numel())
        if stereo_baseline != 0.0:
            check(lib.pvo_ba_rig(*args, _vp(disps_sens), float(alpha), stereo_baseline, _stream(dev)), "ba (stereo)")
        elif disps_sens is None:
            check(lib.pvo_ba(*args, _stream(dev)), "ba")
        else:
            check(lib.pvo_ba_prior(*args, _ptr(disps_sens), float(alpha), _stream(dev)), "ba (sensor depth)")
    return [dx, dz]


# --------------------------------------------------------------------------- edge-sharded BA pieces
def ba_workspace_bytes(E, P, nframes, HW):
    return int(_lib.load().pvo_ba_workspace_bytes(int(E), int(P), int(nframes), int(HW)))


def ba_workspace(E, P, nframes, HW, device):
    """a private workspace tensor for the split BA entry points (one per rank / graph)"""
    n = _lib.load().pvo_ba_workspace_bytes(int(E), int(P), int(nframes), int(HW))
    return torch.empty(int(n), dtype=torch.uint8, device=device)


def ba_last_partition(E, P, nframes, HW, device, workspace=None):
    """diagnostic: (m, s) of the partitioned pose solve the last BA of this size ran with on `device` - poses [0, m) and
    [s, P) were eliminated by two workgroups at once, the separator [m, s) last; (0, 0) = one chain.  `workspace`: the
    private workspace of the split entry points, default the one `ba` uses.  Synchronises."""
    dev = torch.device(device)
    lib = _lib.load()
    ws = workspace if workspace is not None else _workspace(dev, lib.pvo_ba_workspace_bytes(int(E), int(P), int(nframes), int(HW)))
    out = (ctypes.c_int * 2)()
    with torch.cuda.device(dev):
        check(lib.pvo_ba_last_partition(ctypes.c_void_p(ws.data_ptr()), ws.numel(), int(E), int(P), int(nframes), int(HW), out, _stream(dev)),
              "ba_last_partition")
    return int(out[0]), int(out[1])


def ba_plan(ii, jj, nframes, HW, K_eta, t0, t1, workspace):
    dev = _dev(ii, jj, workspace)
    _long(ii, "ii"); _long(jj, "jj")
    with torch.cuda.device(dev):
        check(_lib.load().pvo_ba_plan(_ptr(ii), _ptr(jj), ii.shape[0], int(nframes), int(HW), int(K_eta), int(t0), int(t1),
                                      ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), _stream(dev)), "ba_plan")


def ba_depth_prior(workspace, E, P, nframes, HW, disps_sens, alpha=0.05):
    """the sensor-depth prior of every later ba_local on this PLANNED workspace (pvo_ba_depth_prior): disps_sens [nframes,ht,wd]
    fp32, 0 = no measurement; None clears it, and so does the next ba_plan.  The map is read at every step: keep it alive."""
    if disps_sens is not None:
        _f32(disps_sens, "disps_sens")
        _contig(disps_sens, "disps_sens")
        if disps_sens.numel() != int(nframes) * int(HW):
            raise PvoHipError("ba_depth_prior: disps_sens must hold nframes x HW = %d x %d values" % (nframes, HW))
    dev = _dev(workspace, disps_sens)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_ba_depth_prior(ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), int(E), int(P), int(nframes), int(HW),
                                             _ptr(disps_sens), float(alpha), _stream(dev)), "ba_depth_prior")


def ba_stereo(workspace, E, P, nframes, HW, baseline):
    """the stereo baseline of every later ba_local on this PLANNED workspace (pvo_ba_stereo): with baseline > 0 an edge (i, i) is a
    stereo edge; 0 clears it, and so does the next ba_plan."""
    dev = _dev(workspace)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_ba_stereo(ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), int(E), int(P), int(nframes), int(HW),
                                        _baseline(baseline, "ba_stereo"), _stream(dev)), "ba_stereo")


BA_SIGMA_MAX_POSES = 64      # pvo_ba_sigma / pvo_ba_uncertainty: the frontend's window (include/pvo_hip.h)


def _sigma_outputs(P, disps, var_cond, var_pose, status, what):
    """pose_cov [6P,6P] fp64 (fresh) and the two caller-provided variance maps checked: fp32, contiguous, disps' shape"""
    if P > BA_SIGMA_MAX_POSES:
        raise PvoHipError("%s: at most %d window poses (got %d)" % (what, BA_SIGMA_MAX_POSES, P))
    for t, n in ((var_cond, "var_cond"), (var_pose, "var_pose")):
        if t is None:
            continue
        _f32(t, n)
        _contig(t, n)
        if tuple(t.shape) != tuple(disps.shape) or t.device != disps.device:
            raise PvoHipError("%s: %s must have disps' shape %s and device" % (what, n, tuple(disps.shape)))
    _status4(status, what)
    return torch.zeros(6 * P, 6 * P, dtype=torch.float64, device=disps.device)


def ba_sigma(sys, workspace, ii, jj, disps, t0, t1, lm, ep, var_cond=None, var_pose=None, status=None):
    """depth and pose uncertainty of the step `ba_local(..., motion_only=False, sys, workspace)` has just assembled on a planned
    workspace (pvo_ba_sigma, include/pvo_hip.h).  disps [F,ht,wd] gives the shapes only.  var_cond / var_pose [F,ht,wd] fp32
    (optional) are written IN PLACE on the rows unique([t0,t1) U ii); returns pose_cov as a [P,6,P,6] fp64 view of the symmetric
    [6P,6P] inverse of the damped pose system.  Nothing of sys or the plan is modified.  No host synchronisation."""
    for t, n in ((ii, "ii"), (jj, "jj"), (sys, "sys")):
        _contig(t, n)
    _long(ii, "ii"); _long(jj, "jj")
    dev = _dev(sys, workspace, ii, jj, disps, var_cond, var_pose, status)
    F, ht, wd = disps.shape
    t0, t1 = int(t0), int(t1)
    P = t1 - t0
    if P < 0 or t0 < 0 or t1 > F:
        raise PvoHipError("ba_sigma: pose window [%d,%d) exceeds the %d depth maps" % (t0, t1, F))
    if sys.dtype != torch.int64 or sys.numel() < (6 * P) ** 2 + 6 * P:
        raise PvoHipError("ba_sigma: sys must be int64 with (6P)^2 + 6P elements")
    cov = _sigma_outputs(P, disps, var_cond, var_pose, status, "ba_sigma")
    with torch.cuda.device(dev):
        check(_lib.load().pvo_ba_sigma(_ptr(sys), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), _ptr(ii), _ptr(jj),
                                       ii.shape[0], P, F, ht, wd, t0, float(lm), float(ep), _ptr(cov), _vp(var_cond), _vp(var_pose),
                                       _vp(status), _stream(dev)), "ba_sigma")
    return cov.view(P, 6, P, 6)


def ba_uncertainty(poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, lm, ep, var_cond=None, var_pose=None,
                   status=None, disps_sens=None, alpha=0.05, stereo_baseline=0.0):
    """the one-call form (pvo_ba_uncertainty): `ba`'s operands of ONE depth-BA step, read only.  var_cond / var_pose [F,ht,wd]
    fp32 (optional) are written IN PLACE on the rows unique([t0,t1) U ii); returns pose_cov [P,6,P,6] fp64.  disps_sens / alpha /
    stereo_baseline as in `ba`.  status (optional int32[4]) receives [failed, K, eta-row mismatch, row-table overflow of the elimination].  No host synchronisation."""
    stereo_baseline = _baseline(stereo_baseline, "ba_uncertainty")
    if disps_sens is not None:
        _sens_map(disps_sens, disps, "ba_uncertainty")
    dev, F, ht, wd, HW, E, t0, t1, P = _ba_operands("ba_uncertainty", poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1,
                                                    var_cond, var_pose, status)
    eta = eta.contiguous().view(-1, HW)
    cov = _sigma_outputs(P, disps, var_cond, var_pose, status, "ba_uncertainty")
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_ba_workspace_bytes(E, P, F, HW))
    with torch.cuda.device(dev):
        check(lib.pvo_ba_uncertainty(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(targets), _ptr(weights), _ptr(eta), _ptr(ii), _ptr(jj),
                                     E, F, ht, wd, eta.shape[0], t0, t1, float(lm), float(ep), _ptr(cov), _vp(var_cond), _vp(var_pose),
                                     _vp(status), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _vp(disps_sens), float(alpha),
                                     stereo_baseline, _stream(dev)), "ba_uncertainty")
    return cov.view(P, 6, P, 6)


BA_CALIB_MAX_POSES = 64      # pvo_ba_calib: the frontend's window (include/pvo_hip.h)
BA_CALIB_FREE = {"all": 15, "focal": 3}
_calib_ws_cache = {}


def ba_calib(poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, ep_c=0.1, free_mask=15, status=None):
    """the calibrating depth BA (pvo_ba_calib, include/pvo_hip.h): `ba`'s operands with intrinsics [4] fp32 UPDATED IN PLACE beside
    poses and disps.  free_mask: bit n frees (fx, fy, cx, cy)[n]; a held parameter keeps its bytes.  Returns [dx [P,6], dz [K,ht*wd],
    dc [4]] of the last step (zeros when it was rejected).  status (optional int32[4]) receives [a step was rejected, K, eta-row
    mismatch, row-table overflow].  1 <= P <= BA_CALIB_MAX_POSES.  Runs on the workspace `ba` uses.  No host synchronisation."""
    dev, F, ht, wd, HW, E, t0, t1, P = _ba_operands("ba_calib", poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, status)
    if P > BA_CALIB_MAX_POSES:
        raise PvoHipError("ba_calib: at most %d window poses (got %d)" % (BA_CALIB_MAX_POSES, P))
    if intrinsics.numel() != 4:
        raise PvoHipError("ba_calib: intrinsics must hold the 4 values fx, fy, cx, cy")
    _status4(status, "ba_calib")
    eta = eta.contiguous().view(-1, HW)
    K_eta = eta.shape[0]
    K = _depth_rows(K_eta, t0, t1, ii, dev)
    dx = torch.zeros(max(P, 0), 6, dtype=torch.float32, device=dev)
    dz = torch.zeros(K, HW, dtype=torch.float32, device=dev)
    dc = torch.zeros(4, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = _workspace(dev, lib.pvo_ba_workspace_bytes(E, P, F, HW))
    nb = lib.pvo_ba_calib_workspace_bytes(E, P, F, HW)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    cws = _calib_ws_cache.get(key)
    if cws is None or cws.numel() < nb:
        cws = _calib_ws_cache[key] = torch.empty(int(nb) + (int(nb) >> 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.pvo_ba_calib(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(targets), _ptr(weights), _ptr(eta), _ptr(ii), _ptr(jj),
                               E, F, ht, wd, K_eta, t0, t1, int(iterations), float(lm), float(ep), float(ep_c), int(free_mask),
                               _ptr(dx), _ptr(dz), K, _ptr(dc), _vp(status), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                               ctypes.c_void_p(cws.data_ptr()), cws.numel(), _stream(dev)), "ba_calib")
    return [dx, dz, dc]


def depth_sense(depth, out_row):
    """RGB-D ingest (pvo_depth_sense): out_row [H/8,W/8] fp32 = 1 / depth[3::8, 3::8] where that is finite and > 0, else 0.
    depth [H,W] fp32 / fp16 on the device; one launch."""
    dev = _dev(depth, out_row)
    _contig(depth, "depth"); _contig(out_row, "out_row")
    _f32(out_row, "out_row")
    if depth.dim() != 2 or tuple(out_row.shape) != (depth.shape[0] // 8, depth.shape[1] // 8):
        raise PvoHipError("depth_sense: depth [H,W] and out_row [H/8,W/8] expected, got %s and %s" % (tuple(depth.shape), tuple(out_row.shape)))
    if depth.dtype not in (torch.float32, torch.float16):
        raise PvoHipError("depth_sense: depth must be float32 or float16")
    with torch.cuda.device(dev):
        check(_lib.load().pvo_depth_sense(_ptr(depth), _ptr(out_row), depth.shape[0], depth.shape[1], _DT[depth.dtype], _stream(dev)),
              "depth_sense")
    return out_row


BA_SYS_DTYPE = torch.int64      # the reduced pose system is 64-bit fixed point (units of 2^-28): all-reduce it as integers


def ba_local(poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, motion_only, sys, workspace, sys_is_zero=False):
    """assemble + eliminate this rank's edges; `sys` (int64 [(6P)^2+6P], fixed point) receives the local reduced system.
    sys_is_zero: the buffer was left zeroed by ba_finish (skips the clear)."""
    dev = _dev(poses, disps, intrinsics, targets, weights, eta, ii, jj, sys, workspace)
    F, ht, wd = disps.shape
    if sys.dtype != torch.int64 or sys.numel() < (6 * (t1 - t0)) ** 2 + 6 * (t1 - t0):
        raise PvoHipError("ba_local: sys must be int64 with (6P)^2 + 6P elements")
    K_eta = 1
    if eta is not None:
        eta = eta.contiguous().view(-1, ht * wd)
        K_eta = eta.shape[0]
    with torch.cuda.device(dev):
        check(_lib.load().pvo_ba_local(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(targets), _ptr(weights),
                                       _vp(eta), _ptr(ii), _ptr(jj),
                                       ii.shape[0], F, ht, wd, K_eta, int(t0), int(t1), (1 if motion_only else 0) | (2 if sys_is_zero else 0),
                                       _ptr(sys), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(),
                                       _stream(dev)), "ba_local")


def ba_packed_elems(first):
    """int64 elements of the packed envelope message for the structural envelope `first` (a host list, one entry per free pose)"""
    arr = (ctypes.c_int * len(first))(*[int(f) for f in first])
    return int(_lib.load().pvo_ba_packed_elems(arr, len(first)))


def ba_pack(sys, first_dev, msg):
    """after ba_local: the structural envelope (first_dev: int32 [P] on the device) of `sys` -> msg (int64, ba_packed_elems long);
    `sys` is left zeroed.  msg is what an edge-sharded step all-reduces; ba_finish(..., packed=(msg, first_dev)) consumes it."""
    dev = _dev(sys, first_dev, msg)
    if sys.dtype != torch.int64 or msg.dtype != torch.int64 or first_dev.dtype != torch.int32:
        raise PvoHipError("ba_pack: sys / msg must be int64, first int32")
    with torch.cuda.device(dev):
        check(_lib.load().pvo_ba_pack(_ptr(sys), _ptr(first_dev), _ptr(msg), int(first_dev.shape[0]), _stream(dev)), "ba_pack")
    return msg


BA_SOLVE_KINDS = ("status", "dense", "envelope", "chain", "blocks")


def ba_solve_kind(P, graph_edges, packed=False):
    """the form ba_finish factorises the reduced pose system with (pvo_ba_solve_kind: the host-side rule, no GPU), a name of
    BA_SOLVE_KINDS, from what the rule reads: the free poses, the WHOLE graph's edge count, whether the system is a packed message"""
    k = int(_lib.load().pvo_ba_solve_kind(int(P), int(graph_edges), 1 if packed else 0))
    if k < 0:
        raise PvoHipError("ba_solve_kind: P and graph_edges must not be negative")
    return BA_SOLVE_KINDS[k]


def ba_finish(poses, disps, sys, ii, jj, t0, t1, lm, ep, motion_only, workspace, dz_rows=0, status=None, outputs=True,
              clamp_frames=0, disp_min=0.001, rider=None, packed=None, graph_edges=None):
    """damp + solve the (all-reduced) system (left zeroed afterwards), retract poses, back-substitute this rank's depths -> [dx, dz]
    (outputs=False: poses / disps are updated in place and no dx / dz tensors are produced -> [None, None]).
    clamp_frames > 0: disps[:clamp_frames].clamp_(min=disp_min) in the same launch.
    rider = (x, w, bias): an independent 1x1 convolution of x [N,128,H,W] (conv1x1_c128 without ReLU) computed by additional
    workgroups of the pose solve's dispatch (pvo_ba_finish_conv1x1); its result is appended to the returned list.
    packed = (msg, first_dev): the all-reduced envelope message of ba_pack instead of the dense `sys` (which is not read).
    graph_edges: the edge count of the WHOLE graph where ii / jj are a shard of it and `sys` was all-reduced densely
    (pvo_ba_finish_graph) - the solve form is chosen from it, so every rank chooses alike; None: ii / jj are the whole graph."""
    dev = _dev(poses, disps, sys, ii, jj, workspace)
    rx = rw = rb = ry = None
    rrows = rC = rdt = 0
    if rider is not None:
        rx, rw, rb = rider
        _cl(rx, "rider x", 128)
        if rw.dim() != 2 or rw.shape[1] != 128 or rw.dtype != rx.dtype or not rw.is_contiguous():
            raise PvoHipError("ba_finish: rider w must be a contiguous [Cout,128] tensor in x's dtype")
        rC = rw.shape[0]
        ry = _new_cl(rx.shape[0], rC, rx.shape[2], rx.shape[3], rx.dtype, dev)
        rrows, rdt = rx.shape[0] * rx.shape[2] * rx.shape[3], _dtype_code(rx, "rider x")
    F, ht, wd = disps.shape
    P = int(t1) - int(t0)
    dx = torch.zeros(max(P, 0), 6, dtype=torch.float32, device=dev) if outputs else None
    dz = torch.zeros(int(dz_rows), ht * wd, dtype=torch.float32, device=dev) if outputs else None
    if not outputs:
        dz_rows = 0
    lib = _lib.load()
    # what every finish entry point takes behind its system (sys, or msg + first) and in front of its own tail
    common = (_ptr(ii), _ptr(jj), ii.shape[0], F, ht, wd,
              int(t0), int(t1), float(lm), float(ep), 1 if motion_only else 0,
              int(clamp_frames), float(disp_min), _ptr(dx), _ptr(dz), int(dz_rows), _vp(status),
              ctypes.c_void_p(workspace.data_ptr()), workspace.numel())
    if packed is not None:
        msg, first_dev = packed
        if rider is not None:
            raise PvoHipError("ba_finish: a rider and a packed message together are not supported")
        if msg.dtype != torch.int64 or first_dev.dtype != torch.int32 or first_dev.shape[0] != P:
            raise PvoHipError("ba_finish: packed = (int64 message, int32 [P] structural envelope)")
        with torch.cuda.device(dev):
            check(lib.pvo_ba_finish_packed(_ptr(poses), _ptr(disps), _ptr(msg), _ptr(first_dev), *common, _stream(dev)), "ba_finish_packed")
        return [dx, dz]
    if graph_edges is not None:
        if rider is not None:
            raise PvoHipError("ba_finish: a rider and graph_edges together are not supported")
        with torch.cuda.device(dev):
            check(lib.pvo_ba_finish_graph(_ptr(poses), _ptr(disps), _ptr(sys), *common, int(graph_edges), _stream(dev)), "ba_finish_graph")
        return [dx, dz]
    with torch.cuda.device(dev):
        check(lib.pvo_ba_finish_conv1x1(
            _ptr(poses), _ptr(disps), _ptr(sys), *common,
            _ptr(rx), _ptr(rw), _bias(rb, rC, "rider bias") if rider is not None else None, _ptr(ry),
            int(rrows), int(rC), int(rdt), _stream(dev)), "ba_finish")
    return [dx, dz] if rider is None else [dx, dz, ry]


# --------------------------------------------------------------------------- update operator layers
def _cl(t, name, C):
    """a [E,C,H,W] tensor stored channels-last (physically [E,H,W,C]), 16-bit"""
    if t.dim() != 4 or t.shape[1] != C or not t.is_contiguous(memory_format=torch.channels_last):
        raise PvoHipError("%s must be a channels-last [E,%d,H,W] tensor" % (name, C))
    if t.dtype not in (torch.float16, torch.bfloat16):
        raise PvoHipError("%s must be float16 or bfloat16" % name)


def _bias(b, C, what):
    if b is None:
        return ctypes.c_void_p(0)
    if b.dtype != torch.float32 or b.numel() != C or not b.is_contiguous() or not b.is_cuda:
        raise PvoHipError("%s must be a contiguous float32 device vector of %d elements" % (what, C))
    return _ptr(b)


def _new_cl(E, C, H, W, dtype, dev):
    return torch.empty(E, H, W, C, dtype=dtype, device=dev).permute(0, 3, 1, 2)


def gru_glo_fused(net, w_weight, w_bias=None):
    """global context with the 1x1 conv folded in, as partial means over 256-pixel chunks:
    returns [E, K, 128] f32 with mean_px sigmoid(w(net) + b) * net == result.sum(1).
    net [E,128,H,W] channels-last 16-bit; w_weight [128,128] (or [128,128,1,1]) in net's dtype."""
    _cl(net, "net", 128)
    dev = _dev(net, w_weight)
    E, C, H, W = net.shape
    w2d = w_weight.reshape(128, 128)
    if w2d.dtype != net.dtype or not w2d.is_contiguous():
        raise PvoHipError("gru_glo_fused: w_weight must be a contiguous [128,128] tensor in net's dtype")
    lib = _lib.load()
    part = torch.empty(E, lib.pvo_gru_glo_chunks(H * W), C, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.pvo_gru_glo_fused(_ptr(net), _ptr(w2d), _bias(w_bias, C, "w_bias"), _ptr(part), E, H * W,
                                    _dtype_code(net, "net"), _stream(dev)), "gru_glo_fused")
    return part


def gate_context(glo_part, wg_t, g_bias):
    """g [E,384] f32 = (sum over chunks of glo_part [E,K,128]) @ wg_t [128,384] + g_bias [384]: the ConvGRU's three
    global-context 1x1 convolutions (gru.py:13-15) with every per-channel bias of the gates folded in"""
    dev = _dev(glo_part, wg_t, g_bias)
    E, K, C = glo_part.shape
    for t, n in ((glo_part, "glo_part"), (wg_t, "wg_t"), (g_bias, "g_bias")):
        _f32(t, n); _contig(t, n)
    if C != 128 or tuple(wg_t.shape) != (128, 384) or g_bias.numel() != 384:
        raise PvoHipError("gate_context: glo_part [E,K,128], wg_t [128,384], g_bias [384]")
    g = torch.empty(E, 384, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_gate_context(_ptr(glo_part), _ptr(wg_t), _ptr(g_bias), _ptr(g), E, K, _stream(dev)), "gate_context")
    return g


def conv7x7_c8_weights(weight, dtype):
    """[128,8,7,7] conv filter -> the [52,128,8] tap-major layout pvo_conv7x7_c8 reads (3 zero taps of padding)"""
    co, ci, kh, kw = weight.shape
    if (co, ci, kh, kw) != (128, 8, 7, 7):
        raise PvoHipError("conv7x7_c8: filter must be [128,8,7,7]")
    w = torch.zeros(52, 128, 8, dtype=dtype, device=weight.device)
    w[:49] = weight.detach().permute(2, 3, 0, 1).reshape(49, 128, 8).to(dtype)
    return w.contiguous()


def conv7x7_c8(x, w_taps, bias):
    """relu(conv7x7(x) + bias): x [E,8,H,W] channels-last 16-bit -> [E,128,H,W] channels-last (flow_encoder[0:2])"""
    _cl(x, "x", 8)
    dev = _dev(x, w_taps, bias)
    E, _, H, W = x.shape
    if w_taps.dtype != x.dtype or tuple(w_taps.shape) != (52, 128, 8) or not w_taps.is_contiguous():
        raise PvoHipError("conv7x7_c8: w_taps must be the [52,128,8] tensor of conv7x7_c8_weights in x's dtype")
    y = _new_cl(E, 128, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_conv7x7_c8(_ptr(x), _ptr(w_taps), _bias(bias, 128, "bias"), _ptr(y), E, H, W,
                                         _dtype_code(x, "x"), _stream(dev)), "conv7x7_c8")
    return y


def flow_encoder(x, w7_taps, bias7, w3_taps, bias3, out=None, out_offset=0):
    """relu(conv3x3(relu(conv7x7(x) + bias7)) + bias3) in one kernel (pvo_flow_encoder): x [E,8,H,W] channels-last 16-bit ->
    [E,64,H,W] channels-last, or a channel slice of `out`"""
    _cl(x, "x", 8)
    dev = _dev(x, w7_taps, bias7, w3_taps, out)
    E, _, H, W = x.shape
    if w7_taps.dtype != x.dtype or tuple(w7_taps.shape) != (52, 128, 8) or not w7_taps.is_contiguous():
        raise PvoHipError("flow_encoder: w7_taps must be the [52,128,8] tensor of conv7x7_c8_weights in x's dtype")
    if tuple(w3_taps.shape) != (9, 64, 128) or w3_taps.dtype != x.dtype or not w3_taps.is_contiguous():
        raise PvoHipError("flow_encoder: w3_taps must be the [9,64,128] tensor of conv3x3_c128_weights in x's dtype")
    ret, y, ys, yo = _out_slice(out, out_offset, E, 64, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_flow_encoder(_ptr(x), _ptr(w7_taps), _bias(bias7, 128, "bias7"), _ptr(w3_taps), _bias(bias3, 64, "bias3"),
                                           _ptr(y), E, H, W, ys, yo, _dtype_code(x, "x"), _stream(dev)), "flow_encoder")
    return ret


def conv3x3_c128_weights(weight, dtype):
    """[Cout,128,3,3] conv filter -> the [9,Cout,128] tap-major layout pvo_conv3x3_c128 reads"""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (3, 3):
        raise PvoHipError("conv3x3: filter must be [Cout,Cin,3,3]")
    return weight.detach().permute(2, 3, 0, 1).reshape(9, co, ci).to(dtype).contiguous()


def conv3x3_weights(weight, dtype):
    """[Cout,Cin,3,3] conv filter (Cin % 32 == 0, Cout % 128 == 0) -> the layout pvo_conv3x3 / pvo_gru_conv_* read, as a
    [9,Cout,Cin]-shaped tensor holding MFMA-fragment order [Cout/128][Cin/32][9][2][4][64][8] (include/pvo_hip.h)"""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or ci % 32 or co % 128:
        raise PvoHipError("conv3x3: filter must be [Cout,Cin,3,3] with Cin % 32 == 0 and Cout % 128 == 0")
    taps = weight.detach().permute(2, 3, 0, 1).reshape(9, co, ci).to(dtype)
    # (t, cg, wn, nt, li, cc, kg, j) -> (cg, cc, t, wn, nt, kg, li, j): lane = kg * 16 + li of v_mfma_f32_16x16x32
    f = taps.reshape(9, co // 128, 2, 4, 16, ci // 32, 4, 8).permute(1, 5, 0, 2, 3, 6, 4, 7)
    return f.contiguous().view(9, co, ci)


def _out_slice(out, out_offset, E, Cout, H, W, dtype, dev):
    """(tensor to return, pointer tensor, ystride, yoff): a fresh dense output, or a channel slice of `out`"""
    if out is None:
        y = _new_cl(E, Cout, H, W, dtype, dev)
        return y, y, 0, 0
    if out.dim() != 4 or out.shape[0] != E or tuple(out.shape[2:]) != (H, W) or out.dtype != dtype or \
            not out.is_contiguous(memory_format=torch.channels_last) or out_offset < 0 or out_offset + Cout > out.shape[1]:
        raise PvoHipError("out must be a channels-last [E,C>=offset+Cout,H,W] tensor of the input dtype")
    return out[:, out_offset:out_offset + Cout], out, out.shape[1], out_offset


def conv3x3(x, w_taps, bias=None, relu=False, out=None, out_offset=0):
    """act(conv3x3(x) + bias): x [E,Cin,H,W] channels-last 16-bit -> [E,Cout,H,W] channels-last (wide layers: Cin % 32
    == 0, Cout % 128 == 0).  out / out_offset: write into channels [out_offset, out_offset + Cout) of `out`."""
    dev = _dev(x, w_taps, out)
    E, Cin, H, W = x.shape
    _cl(x, "x", Cin)
    if w_taps.dim() != 3 or w_taps.shape[0] != 9 or w_taps.shape[2] != Cin or w_taps.dtype != x.dtype or not w_taps.is_contiguous():
        raise PvoHipError("conv3x3: w_taps must be the [9,Cout,Cin] tensor of conv3x3_weights in x's dtype")
    Cout = w_taps.shape[1]
    ret, y, ys, yo = _out_slice(out, out_offset, E, Cout, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_conv3x3(_ptr(x), _ptr(w_taps), _bias(bias, Cout, "bias"), _ptr(y), E, H, W, Cin, Cout,
                                      1 if relu else 0, ys, yo, _dtype_code(x, "x"), _stream(dev)), "conv3x3")
    return ret


def conv3x3_c128(x, w_taps, bias=None, relu=False, out=None, out_offset=0):
    """act(conv3x3(x) + bias): x [E,128,H,W] channels-last 16-bit -> [E,Cout,H,W] channels-last, Cout in {64,128,256,512}"""
    _cl(x, "x", 128)
    dev = _dev(x, w_taps, out)
    E, _, H, W = x.shape
    if w_taps.dim() != 3 or w_taps.shape[0] != 9 or w_taps.shape[2] != 128 or w_taps.dtype != x.dtype or not w_taps.is_contiguous():
        raise PvoHipError("conv3x3_c128: w_taps must be the [9,Cout,128] tensor of conv3x3_weights in x's dtype")
    Cout = w_taps.shape[1]
    ret, y, ys, yo = _out_slice(out, out_offset, E, Cout, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_conv3x3_c128(_ptr(x), _ptr(w_taps), _bias(bias, Cout, "bias"), _ptr(y), E, H, W, Cout,
                                           1 if relu else 0, ys, yo, _dtype_code(x, "x"), _stream(dev)), "conv3x3_c128")
    return ret


def gru_conv_gates(net, cf, w_taps, g, P_zr, p_slots=None):
    """gate convolution over [net | cf] + sigmoid gates in one kernel -> (Z, RN), each [E,128,H,W] channels-last.
    cf [E,C,H,W] (C % 32 == 0), w_taps [9,256,128+C], g [E,384] f32, P_zr [E,256,H,W]."""
    E, _, H, W = net.shape
    C = cf.shape[1]
    _cl(net, "net", 128); _cl(cf, "cf", C); _cl(P_zr, "P_zr", 256)
    dev = _dev(net, cf, w_taps, g, P_zr, p_slots)
    if p_slots is not None and (p_slots.dtype != torch.int32 or p_slots.numel() != E or not p_slots.is_contiguous()):
        raise PvoHipError("gru_conv_gates: p_slots must be a contiguous int32 [E] tensor")
    _f32(g, "g"); _contig(g, "g")
    if tuple(w_taps.shape) != (9, 256, 128 + C) or w_taps.dtype != net.dtype or not w_taps.is_contiguous():
        raise PvoHipError("gru_conv_gates: w_taps must be [9,256,128+C] in net's dtype")
    Z, RN = _new_cl(E, 128, H, W, net.dtype, dev), _new_cl(E, 128, H, W, net.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_gru_conv_gates(_ptr(net), _ptr(cf), C, _ptr(w_taps), _ptr(g), _ptr(P_zr), _vp(p_slots), _ptr(Z), _ptr(RN),
                                             E, H, W, _dtype_code(net, "net"), _stream(dev)), "gru_conv_gates")
    return Z, RN


def gru_conv_candidate(RN, cf, w_taps, g, P_q, Z, net, p_slots=None):
    """candidate convolution over [RN | cf] + the GRU state update in one kernel -> new hidden state"""
    E, _, H, W = net.shape
    C = cf.shape[1]
    _cl(RN, "RN", 128); _cl(cf, "cf", C); _cl(P_q, "P_q", 128); _cl(Z, "Z", 128); _cl(net, "net", 128)
    dev = _dev(RN, cf, w_taps, g, P_q, Z, net)
    _f32(g, "g"); _contig(g, "g")
    if tuple(w_taps.shape) != (9, 128, 128 + C) or w_taps.dtype != net.dtype or not w_taps.is_contiguous():
        raise PvoHipError("gru_conv_candidate: w_taps must be [9,128,128+C] in net's dtype")
    out = _new_cl(E, 128, H, W, net.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_gru_conv_candidate(_ptr(RN), _ptr(cf), C, _ptr(w_taps), _ptr(g), _ptr(P_q), _vp(p_slots), _ptr(Z), _ptr(net),
                                                 _ptr(out), E, H, W, _dtype_code(net, "net"), _stream(dev)), "gru_conv_candidate")
    return out


def corr_encode(corr, enc_weight, enc_bias):
    """relu(W corr + b): corr [E,196,H,W] channels-last 16-bit -> [E,128,H,W] channels-last (corr_encoder[0:2])"""
    _cl(corr, "corr", 196)
    dev = _dev(corr, enc_weight, enc_bias)
    E, _, H, W = corr.shape
    if tuple(enc_weight.shape) != (128, 224) or enc_weight.dtype != corr.dtype or not enc_weight.is_contiguous():
        raise PvoHipError("enc_weight must be the [128,224] tensor of corr_encoder_weights in the feature dtype")
    y = _new_cl(E, 128, H, W, corr.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_corr_encode(_ptr(corr), _ptr(enc_weight), _bias(enc_bias, 128, "enc_bias"), _ptr(y), E * H * W,
                                          _dtype_code(corr, "corr"), _stream(dev)), "corr_encode")
    return y


def segment_mean(x, seg_ptr, seg_idx, K, in_bias=None):
    """out[k] = mean of x[seg_idx[e]] for e in [seg_ptr[k], seg_ptr[k+1]); x channels-last [E,C,H,W] -> [K,C,H,W].
    in_bias (f32 [C]): average relu(x + in_bias) instead (x = a bias-free convolution output)."""
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last) or x.dtype not in (torch.float16, torch.bfloat16):
        raise PvoHipError("segment_mean: x must be a channels-last 16-bit [E,C,H,W] tensor")
    dev = _dev(x, seg_ptr, seg_idx)
    if seg_ptr.dtype != torch.int32 or seg_idx.dtype != torch.int32:
        raise PvoHipError("segment_mean: seg_ptr / seg_idx must be int32")
    E, C, H, W = x.shape
    out = _new_cl(K, C, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_segment_mean(_ptr(x), _ptr(seg_ptr), _ptr(seg_idx), _bias(in_bias, C, "in_bias"), _ptr(out), K, H * W, C,
                                           _dtype_code(x, "x"), _stream(dev)), "segment_mean")
    return out


def heads_out(h1, bias1, w2, bias2):
    """y [E,8,H,W] (channels-last) = the four heads' second 3x3 convolutions of relu(h1 + bias1);
    h1 [E,512,H,W] channels-last 16-bit, w2 [4,2,9,128] same dtype, bias1 [512] / bias2 [8] float32"""
    _cl(h1, "h1", 512)
    dev = _dev(h1, bias1, w2, bias2)
    if tuple(w2.shape) != (4, 2, 9, 128) or w2.dtype != h1.dtype or not w2.is_contiguous():
        raise PvoHipError("heads_out: w2 must be a contiguous [4,2,9,128] tensor of the feature dtype")
    E, _, H, W = h1.shape
    y = _new_cl(E, 8, H, W, h1.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_heads_out(_ptr(h1), _bias(bias1, 512, "bias1"), _ptr(w2), _bias(bias2, 8, "bias2"), _ptr(y),
                                        E, H, W, _dtype_code(h1, "h1"), _stream(dev)), "heads_out")
    return y


def heads2_fragments(w2, dtype):
    """second-stage filter of the four heads, [4,2,9,128] ([head][out][tap][channel]), as the MFMA B fragments
    pvo_conv3x3_heads multiplies the hidden activations with: [4][8 k-steps][64 lanes][8], column n = 2 tap + out"""
    w = w2.detach().to(dtype)
    m = torch.zeros(4, 32, 128, dtype=dtype, device=w.device)                 # [head][n][k]
    m[:, :18] = w.permute(0, 2, 1, 3).reshape(4, 18, 128)                       # n = tap * 2 + out
    # element (h, ks, lane, j) = m[h][lane & 31][ks*16 + (lane >> 5)*8 + j]
    f = m.reshape(4, 32, 8, 2, 8).permute(0, 2, 3, 1, 4)                        # [h][ks][kg][n][j]
    return f.reshape(4, 8, 64, 8).contiguous()


def heads_fused(x, w1_taps, bias1, w2_frags, bias2):
    """the four output heads from the hidden state in two launches and without the [E,512,H,W] intermediate:
    x [E,128,H,W] channels-last 16-bit, w1_taps = conv3x3_weights of the concatenated first-stage filters [512,128,3,3],
    w2_frags = heads2_fragments(...).  Returns y [E,8,H,W] channels-last as heads_out does."""
    _cl(x, "x", 128)
    dev = _dev(x, w1_taps, bias1, w2_frags, bias2)
    E, _, H, W = x.shape
    if tuple(w1_taps.shape) != (9, 512, 128) or w1_taps.dtype != x.dtype or not w1_taps.is_contiguous() or \
            tuple(w2_frags.shape) != (4, 8, 64, 8) or w2_frags.dtype != x.dtype or not w2_frags.is_contiguous():
        raise PvoHipError("heads_fused: w1_taps must be [9,512,128] and w2_frags [4,8,64,8] in x's dtype")
    z = torch.empty(E, H, W, 4, 18, dtype=torch.float32, device=dev)
    y = _new_cl(E, 8, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        lib = _lib.load()
        check(lib.pvo_conv3x3_heads(_ptr(x), _ptr(w1_taps), _bias(bias1, 512, "bias1"), _ptr(w2_frags), _ptr(z), E, H, W,
                                    _dtype_code(x, "x"), _stream(dev)), "conv3x3_heads")
        check(lib.pvo_heads_gather(_ptr(z), _bias(bias2, 8, "bias2"), _ptr(y), E, H, W, _dtype_code(x, "x"), _stream(dev)), "heads_gather")
    return y


def eta_head(x, w_taps, bias, frame=None, pos=None, damping=None, EP=0.0, eta_scale=0.2):
    """GraphAgg's eta head: x [K,128,H,W] channels-last 16-bit, w_taps [9,128], bias f32 [1].
    frame None -> 0.01 * softplus(conv(x) + bias) [K,H,W] f32 (what GraphAgg returns).
    frame int64 [R], pos int32 [R], damping f32 [buffer,H,W]: also FactorGraph's damping bookkeeping; returns the BA's
    eta [R,H,W] = eta_scale * damping[frame] + EP (see pvo_eta_head)."""
    _cl(x, "x", 128)
    dev = _dev(x, w_taps, bias, frame, pos, damping)
    K, _, H, W = x.shape
    if tuple(w_taps.shape) != (9, 128) or w_taps.dtype != x.dtype or not w_taps.is_contiguous():
        raise PvoHipError("eta_head: w_taps must be [9,128] in x's dtype")
    R = K
    if frame is not None:
        R = frame.shape[0]
        if frame.dtype != torch.int64 or pos.dtype != torch.int32 or pos.shape[0] != R or damping.dtype != torch.float32 \
                or tuple(damping.shape[1:]) != (H, W) or not damping.is_contiguous():
            raise PvoHipError("eta_head: frame int64 [R], pos int32 [R], damping contiguous f32 [*,H,W]")
    eta = torch.empty(R, H, W, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_eta_head(_ptr(x), _ptr(w_taps), _bias(bias, 1, "bias"), _ptr(frame), _ptr(pos), _ptr(damping),
                                       _ptr(eta), R, H, W, float(EP), float(eta_scale), _dtype_code(x, "x"), _stream(dev)), "eta_head")
    return eta


def conv1x1_c128(x, w, bias=None, relu=False):
    """act(conv1x1(x) + bias): x [N,128,H,W] channels-last 16-bit, w [Cout,128] (Cout % 192 == 0) -> [N,Cout,H,W] channels-last"""
    _cl(x, "x", 128)
    dev = _dev(x, w, bias)
    N, _, H, W = x.shape
    if w.dim() != 2 or w.shape[1] != 128 or w.dtype != x.dtype or not w.is_contiguous():
        raise PvoHipError("conv1x1_c128: w must be a contiguous [Cout,128] tensor in x's dtype")
    Cout = w.shape[0]
    y = _new_cl(N, Cout, H, W, x.dtype, dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_conv1x1_c128(_ptr(x), _ptr(w), _bias(bias, Cout, "bias"), _ptr(y), N * H * W, Cout,
                                           1 if relu else 0, _dtype_code(x, "x"), _stream(dev)), "conv1x1_c128")
    return y


# --------------------------------------------------------------------------- FactorGraph.update glue
def graph_motion(target, coords1, delta_dy, raw_mask, dtype):
    """motion features (factor_graph.py:233-237): [1,E,H,W,2] f32 x4 -> [1,E,8,H,W] in `dtype`, stored channels-last"""
    for t, n in ((target, "target"), (coords1, "coords1"), (delta_dy, "delta_dy"), (raw_mask, "raw_mask")):
        _contig(t, n); _f32(t, n)
    dev = _dev(target, coords1, delta_dy, raw_mask)
    _, E, H, W, _ = target.shape
    motn = torch.empty(E, H, W, 8, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_graph_motion(_ptr(target), _ptr(coords1), _ptr(delta_dy), _ptr(raw_mask), _ptr(motn), E, H, W,
                                           _DT[dtype], _stream(dev)), "graph_motion")
    return motn.permute(0, 3, 1, 2)[None]


def reproject_motion(poses, disps, intrinsics, ii, jj, target, delta_dy, raw_mask, dtype, baseline=0.0):
    """reproject + graph_motion in one pass (pvo_reproject_motion) -> coords [E,ht,wd,2], valid [E,ht,wd,1], motion [1,E,8,H,W].
    baseline > 0: pvo_reproject_motion_rig (stereo edges, see reproject)."""
    baseline = _baseline(baseline, "reproject_motion")
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj"), (target, "target"),
                 (delta_dy, "delta_dy"), (raw_mask, "raw_mask")):
        _contig(t, n)
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (target, "target"), (delta_dy, "delta_dy"), (raw_mask, "raw_mask")):
        _f32(t, n)
    dev = _dev(poses, disps, intrinsics, ii, jj, target, delta_dy, raw_mask)
    _long(ii, "ii"); _long(jj, "jj")
    E, ht, wd = ii.shape[0], disps.shape[1], disps.shape[2]
    coords = torch.empty(E, ht, wd, 2, dtype=torch.float32, device=dev)
    valid = torch.empty(E, ht, wd, 1, dtype=torch.float32, device=dev)
    motn = torch.empty(E, ht, wd, 8, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        a = (_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj), _ptr(coords), _ptr(valid),
             _ptr(target), _ptr(delta_dy), _ptr(raw_mask), _ptr(motn), E, ht, wd, _DT[dtype])
        if baseline == 0.0:
            check(_lib.load().pvo_reproject_motion(*a, _stream(dev)), "reproject_motion")
        else:
            check(_lib.load().pvo_reproject_motion_rig(*a, baseline, _stream(dev)), "reproject_motion (stereo)")
    return coords, valid, motn.permute(0, 3, 1, 2)[None]


def segment_hist(segm, raw_mask, heads, max_segments, dy_thresh=0.5):
    """counting half of the panoptic vote (factor_graph.py:256-261): segm int32 [E,H,W] dense labels in [0, max_segments),
    raw_mask [1,E,H,W,2] f32 (BEFORE the update), heads [E,8,H,W] channels-last -> (tot, dyn) int32 [E,max_segments]"""
    _cl(heads, "heads", 8)
    dev = _dev(segm, raw_mask, heads)
    _contig(segm, "segm"); _contig(raw_mask, "raw_mask"); _f32(raw_mask, "raw_mask")
    E, H, W = segm.shape
    if segm.dtype != torch.int32:
        raise PvoHipError("segment_hist: segm must be int32")
    if raw_mask.numel() != E * H * W * 2 or tuple(heads.shape) != (E, 8, H, W):
        raise PvoHipError("segment_hist: raw_mask must hold [E,H,W,2] and heads [E,8,H,W] for segm [E,H,W]")
    tot = torch.empty(E, max_segments, dtype=torch.int32, device=dev)
    dyn = torch.empty(E, max_segments, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_segment_hist(_ptr(segm), _ptr(raw_mask), _ptr(heads), _ptr(tot), _ptr(dyn), E, H * W, int(max_segments),
                                           float(dy_thresh), _dtype_code(heads, "heads"), _stream(dev)), "segment_hist")
    return tot, dyn


def graph_post(coords1, heads, raw_mask, target_ba, weight_ba, dy_thresh=0.5, vote=None):
    """factor_graph.py:249-306 after the update operator.  heads [E,8,H,W] channels-last 16-bit (delta | delta_dy |
    weight | delta_mask); raw_mask [1,E,H,W,2] is updated IN PLACE; target_ba / weight_ba [E,2,H,W] f32 are filled.
    vote = (segm int32 [E,H,W], tot, dyn int32 [E,S], thresh): the panoptic vote of segment_hist is applied.
    Returns (target_cam, delta_dy, weight, full_flow), each [1,E,H,W,2] f32."""
    _cl(heads, "heads", 8)
    _contig(coords1, "coords1"); _contig(raw_mask, "raw_mask"); _contig(target_ba, "target_ba"); _contig(weight_ba, "weight_ba")
    dev = _dev(coords1, heads, raw_mask, target_ba, weight_ba)
    for t, n in ((coords1, "coords1"), (raw_mask, "raw_mask"), (target_ba, "target_ba"), (weight_ba, "weight_ba")):
        _f32(t, n)
    _, E, H, W, _ = coords1.shape
    if tuple(target_ba.shape) != (E, 2, H, W) or tuple(weight_ba.shape) != (E, 2, H, W):
        raise PvoHipError("graph_post: target_ba and weight_ba must be [E,2,H,W] = [%d,2,%d,%d]" % (E, H, W))
    if tuple(raw_mask.shape) != tuple(coords1.shape) or tuple(heads.shape) != (E, 8, H, W):
        raise PvoHipError("graph_post: raw_mask must have coords1's shape [1,E,H,W,2] and heads must be [E,8,H,W]")
    new = lambda: torch.empty(1, E, H, W, 2, dtype=torch.float32, device=dev)
    target, delta_dy, weight, full_flow = new(), new(), new(), new()
    segm = tot = dyn = None
    S, vth = 0, 0.0
    if vote is not None:
        segm, tot, dyn, vth = vote
        S = tot.shape[1]
        if segm.dtype != torch.int32 or tuple(segm.shape) != (E, H, W) or not segm.is_contiguous() or tot.dtype != torch.int32 \
                or tuple(tot.shape) != (E, S) or tuple(dyn.shape) != (E, S) or dyn.dtype != torch.int32:
            raise PvoHipError("graph_post: vote = (segm int32 [E,H,W], tot int32 [E,S], dyn int32 [E,S], thresh)")
    with torch.cuda.device(dev):
        check(_lib.load().pvo_graph_post(_ptr(coords1), _ptr(heads), _ptr(raw_mask), _ptr(target), _ptr(delta_dy), _ptr(weight),
                                         _ptr(target_ba), _ptr(weight_ba), _ptr(full_flow), E, H, W, float(dy_thresh),
                                         _ptr(segm), _ptr(tot), _ptr(dyn), int(S), float(vth),
                                         _dtype_code(heads, "heads"), _stream(dev)), "graph_post")
    return target, delta_dy, weight, full_flow


# --------------------------------------------------------------------------- the operator / the graph update as one call
class PackedWeights:
    """pvo_update_weights + the tensors it points to (kept alive here)"""

    FIELDS = [n for n, _ in _lib.UpdateWeights._fields_[2:]]

    _serial = itertools.count(1)

    def __init__(self, dtype, tensors, flags=0):
        self.dtype, self.tensors, self.flags = dtype, dict(tensors), flags
        self.serial = next(PackedWeights._serial)      # (identity that survives address reuse: FactorGraph's context token)
        st = _lib.UpdateWeights()
        st.dtype, st.flags = _DT[dtype], flags
        dev = None
        for n in self.FIELDS:
            t = self.tensors[n]
            if not t.is_cuda or not t.is_contiguous():
                raise PvoHipError("packed weight %s must be a contiguous device tensor" % n)
            want = torch.float32 if (n.endswith("_b") or n in ("gate_wt",)) else dtype
            if t.dtype != want:
                raise PvoHipError("packed weight %s must be %s" % (n, want))
            dev = t.device if dev is None else dev
            setattr(st, n, t.data_ptr())
        self.struct, self.device = st, dev

    def on_one_stream(self):
        """the same weights with the operator's side chains (aggregation branch, flow encoder) kept on the launch stream: for callers that
        CAPTURE the operator into a HIP graph - a captured fork becomes a parallel branch the runtime runs on a stream of its own choosing"""
        one = self.__dict__.get("_one_stream")
        if one is None:
            flags = (self.flags | _lib.PVO_OP_SINGLE_STREAM) & ~_lib.PVO_OP_ENC_SIDE_STREAM
            one = self if flags == self.flags else PackedWeights(self.dtype, self.tensors, flags)
            self.__dict__["_one_stream"] = one
        return one

    # a derived cache entry: copies / pickles of the owning module rebuild it (ctypes structs with pointers cannot be copied)
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_none, ())


def _none():
    return None


def _vp(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def _fill_operator_args(a, E, H, W, pool_levels, slots, num_slots, coords, corr, motion, net, net_out, inp, P_zr, P_q,
                        agg, heads, eta_rows, eta, upmask):
    a.E, a.H, a.W = E, H, W
    for l in range(4):
        a.levels[l] = pool_levels[l].data_ptr() if pool_levels is not None else None
    a.slots, a.num_slots = _vp(slots), int(num_slots)
    a.coords, a.corr, a.motion = _vp(coords), _vp(corr), _vp(motion)
    a.net, a.net_out, a.inp, a.P_zr, a.P_q = _vp(net), _vp(net_out), _vp(inp), _vp(P_zr), _vp(P_q)
    a.static_by_slot = 0
    if agg is not None:
        a.seg_ptr, a.seg_idx, a.K = agg[0].data_ptr(), agg[1].data_ptr(), int(agg[2])
    else:
        a.seg_ptr, a.seg_idx, a.K = None, None, 0
    a.heads = _vp(heads)
    if eta_rows is not None:
        frame, pos, damping, EP = eta_rows[:4]
        a.eta_frame, a.eta_pos, a.R, a.damping, a.EP = frame.data_ptr(), pos.data_ptr(), int(frame.shape[0]), damping.data_ptr(), float(EP)
        a.eta_scale = float(eta_rows[4]) if len(eta_rows) > 4 else 0.2
    else:
        a.eta_frame, a.eta_pos, a.R, a.damping, a.EP, a.eta_scale = None, None, 0, None, 0.0, 0.2
    a.eta, a.upmask = _vp(eta), _vp(upmask)


_op_ws = {}


def _op_workspace(key, dev, nbytes):
    buf = _op_ws.get(key)
    if buf is None or buf.numel() < nbytes or buf.device != dev:
        buf = _op_ws[key] = torch.empty(int(nbytes) + (int(nbytes) >> 3), dtype=torch.uint8, device=dev)
    return buf


def update_operator(weights, net, motion, inp=None, P=None, pool=None, coords=None, corr=None, agg=None,
                    eta_rows=None, want_eta=True, want_upmask=True, net_out=None, static_rows=None):
    """DynamicUpdateModule.forward (droid_net.py:256-314) on the 16-bit inference path as ONE call into libpvo_hip.

    weights: PackedWeights.  net, inp [E,128,H,W], motion [E,8,H,W], corr [E,196,H,W]: channels-last 16-bit.
    Correlation features come either from `pool` = (tiled level tensors, slots int32 [E], num_slots) + coords [E,H,W,2]
    f32 (the lookup runs fused with the first encoder layer) or from the sampled tensor `corr`.
    P = (P_zr, P_q): cached static-input terms; None -> computed from `inp` for this call.
    static_rows (int32 [E], pvo_update_operator_rows): P holds per-keyframe pools [F,256,H,W] / [F,128,H,W] and edge e reads image
    static_rows[e] (its source frame); the values are not checked.
    agg = (seg_ptr, seg_idx, K) runs GraphAgg; eta_rows = (frame, pos, damping, EP) selects pvo_eta_head's bookkeeping form.
    Returns (net_out, heads [E,8,H,W], eta f32 or None, upmask [K,576,H,W] or None)."""
    _cl(net, "net", 128); _cl(motion, "motion", 8)
    dev = _dev(net, motion, inp, corr, coords)
    if weights.dtype != net.dtype or weights.device != dev:
        raise PvoHipError("update_operator: packed weights are %s on %s, net is %s on %s" % (weights.dtype, weights.device, net.dtype, dev))
    E, _, H, W = net.shape
    levels = slots = None
    num_slots = 0
    if pool is not None:
        levels, slots, num_slots = pool
        if coords is None or tuple(coords.shape) != (E, H, W, 2) or coords.dtype != torch.float32 or not coords.is_contiguous():
            raise PvoHipError("update_operator: coords must be a contiguous f32 [E,H,W,2] tensor")
        if len(levels) != 4 or levels[0].dtype != net.dtype or slots.dtype != torch.int32 or slots.numel() != E:
            raise PvoHipError("update_operator: pool = (4 tiled level tensors in net's dtype, slots int32 [E], num_slots)")
        for l, lv in enumerate(levels):
            if tuple(lv.shape[1:]) != (H, W) + tiled_level_shape(H, W, l) or not lv.is_contiguous():
                raise PvoHipError("update_operator: tiled pyramid level %d has shape %s" % (l, tuple(lv.shape)))
    elif corr is not None:
        _cl(corr, "corr", 196)
    else:
        raise PvoHipError("update_operator: pass pool + coords, or corr")
    P_zr = P_q = None
    if P is not None:
        P_zr, P_q = P
        _cl(P_zr, "P_zr", 256); _cl(P_q, "P_q", 128)
        if static_rows is not None and (static_rows.dtype != torch.int32 or static_rows.numel() != E or not static_rows.is_contiguous()
                                        or static_rows.device != dev):
            raise PvoHipError("update_operator: static_rows must be a contiguous device int32 [E] tensor")
    elif static_rows is not None:
        raise PvoHipError("update_operator: static_rows index the pools P = (P_zr, P_q)")
    elif inp is None:
        raise PvoHipError("update_operator: pass inp or P")
    else:
        _cl(inp, "inp", 128)
    if net_out is None:
        net_out = _new_cl(E, 128, H, W, net.dtype, dev)
    heads = _new_cl(E, 8, H, W, net.dtype, dev)
    K = int(agg[2]) if agg is not None else 0
    eta = upmask = None
    if K > 0:
        if agg[0].dtype != torch.int32 or agg[1].dtype != torch.int32 or agg[1].numel() != E or agg[0].numel() != K + 1:
            raise PvoHipError("update_operator: agg = (seg_ptr int32 [K+1], seg_idx int32 [E], K)")
        if want_eta:
            eta = torch.empty(eta_rows[0].shape[0] if eta_rows is not None else K, H, W, dtype=torch.float32, device=dev)
        if want_upmask:
            upmask = _new_cl(K, 576, H, W, net.dtype, dev)
    a = _lib.OperatorArgs()
    _fill_operator_args(a, E, H, W, levels, slots, num_slots, coords, corr, motion, net, net_out, inp, P_zr, P_q, agg, heads,
                        eta_rows, eta, upmask)
    lib = _lib.load()
    nbytes = lib.pvo_operator_workspace_bytes(E, K, H, W)
    if torch.cuda.is_current_stream_capturing():
        # a call being captured into a HIP graph (pvo_amd/graphs.py) gets a workspace of its own, allocated from the capture's private
        # memory pool: the shared scratch below is re-allocated whenever a later eager call needs more, and a replay would then
        # write into freed memory
        ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    else:
        ws = _op_workspace(("op", dev.index), dev, nbytes)
    with torch.cuda.device(dev):
        if static_rows is None:
            check(lib.pvo_update_operator(ctypes.byref(weights.struct), ctypes.byref(a), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                          _stream(dev)), "update_operator")
        else:
            check(lib.pvo_update_operator_rows(ctypes.byref(weights.struct), ctypes.byref(a), _ptr(static_rows),
                                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)), "update_operator (frame rows)")
    return net_out, heads, eta, upmask


def bias_norm_act(x, bias=None, residual=None, norm=False, eps=1e-5, relu_inner=False, relu_outer=False, out=None, split=None):
    """what sits between two convolutions of an encoder layer, as one kernel (pvo_bias_norm_act): x [N,C,H,W] contiguous 16-bit ->
    relu_outer(residual + relu_inner(instance_norm(x + bias[c]))), every step rounded to x's dtype.  `out` may be x itself.
    split: None = large planes in slices over two launches (pvo_bias_norm_act_split), False = always the one-workgroup-per-plane kernel."""
    dev = _dev(x, bias, residual)
    _contig(x, "x")
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16):
        raise PvoHipError("bias_norm_act: x must be a contiguous 16-bit [N,C,H,W] tensor")
    N, C, H, W = x.shape
    for t, n in ((bias, "bias"), (residual, "residual")):
        if t is not None:
            _contig(t, n)
            if t.dtype != x.dtype:
                raise PvoHipError("bias_norm_act: %s must have x's dtype" % n)
    if bias is not None and bias.numel() != C or residual is not None and residual.shape != x.shape:
        raise PvoHipError("bias_norm_act: bias [C], residual of x's shape")
    y = torch.empty_like(x) if out is None else out
    lib = _lib.load()
    S = lib.pvo_bias_norm_act_slices(H * W) if split is None else (lib.pvo_bias_norm_act_slices(H * W) if split else 0)
    with torch.cuda.device(dev):
        if S > 0 and N * C <= 65535:
            # large planes: S slices per plane over two launches instead of one workgroup per plane (pvo_bias_norm_act_split)
            ws = torch.empty(2 * N * C * S, dtype=torch.float32, device=dev) if norm else None
            check(lib.pvo_bias_norm_act_split(_ptr(x), _vp(bias), _vp(residual), _ptr(y), N * C, C, H * W, 1 if norm else 0, float(eps),
                                              1 if relu_inner else 0, 1 if relu_outer else 0, _dtype_code(x, "x"), _vp(ws), ws.numel() if norm else 0,
                                              _stream(dev)), "bias_norm_act_split")
        else:
            check(lib.pvo_bias_norm_act(_ptr(x), _vp(bias), _vp(residual), _ptr(y), N * C, C, H * W, 1 if norm else 0, float(eps),
                                        1 if relu_inner else 0, 1 if relu_outer else 0, _dtype_code(x, "x"), _stream(dev)), "bias_norm_act")
    return y


def proximity_select(dist, t0, t1, rad, nms, thresh, have_i, have_j):
    """the greedy proximity-edge selection (pvo_proximity_select, a HOST function of the library): dist = float32 numpy array [ni, nj] of
    frame distances (frames t0.., t1..), have_i / have_j = int64 numpy arrays of the existing edges -> (ii, jj) Python lists"""
    import numpy as np
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    ni, nj = dist.shape
    have_i = np.ascontiguousarray(have_i, dtype=np.int64); have_j = np.ascontiguousarray(have_j, dtype=np.int64)
    cap = 2 * (ni * rad + ni * nj) + 2
    out = np.empty((2, cap), dtype=np.int64)
    n = ctypes.c_int(0)
    check(_lib.load().pvo_proximity_select(dist.ctypes.data, ni, nj, int(t0), int(t1), int(rad), int(nms), float(thresh),
                                           have_i.ctypes.data if have_i.size else None, have_j.ctypes.data if have_j.size else None, int(have_i.size),
                                           out[0].ctypes.data, out[1].ctypes.data, cap, ctypes.byref(n)), "proximity_select")
    return out[0, :n.value].tolist(), out[1, :n.value].tolist()


def conv1x1_planes_supported(cin, cout):
    return cin % 32 == 0 and cout % 64 == 0


def conv1x1_planes(x, w, bias=None, stride=1):
    """Conv2d(Cin, Cout, 1, stride) on a contiguous 16-bit NCHW tensor, deterministic (pvo_conv1x1_planes): x [N,Cin,H,W], w [Cout,Cin] or
    [Cout,Cin,1,1], bias [Cout] or None, all of x's dtype -> [N,Cout,(H-1)//stride+1,(W-1)//stride+1]"""
    dev = _dev(x, w, bias)
    _contig(x, "x"); _contig(w, "w")
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16) or w.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise PvoHipError("conv1x1_planes: x contiguous 16-bit [N,Cin,H,W], w and bias of the same dtype")
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if w.numel() != Cout * Cin or (bias is not None and (bias.numel() != Cout or not bias.is_contiguous())):
        raise PvoHipError("conv1x1_planes: w [Cout,Cin], bias [Cout]")
    stride = int(stride)
    y = torch.empty(N, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=x.dtype, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_conv1x1_planes(_ptr(x), _ptr(w), _vp(bias), _ptr(y), N, Cin, Cout, H, W, stride, _dtype_code(x, "x"), _stream(dev)), "conv1x1_planes")
    return y


def conv_planes_supported(ksize, stride, cin, cout):
    """what pvo_conv_planes runs: 3 x 3 (padding 1) with stride 1 or 2, Cin and Cout multiples of 32; the 7 x 7 stride-2 stem (Cin = 3)"""
    return bool(_lib.load().pvo_conv_planes_supported(int(ksize), int(stride), int(cin), int(cout)))


class PackedConvFilter:
    """a Conv2d weight in the fragment order of pvo_conv_planes (conv_planes_pack); `frag` is the device buffer"""
    __slots__ = ("frag", "ksize", "cin", "cout", "dtype")

    def __init__(self, frag, ksize, cin, cout, dtype):
        self.frag, self.ksize, self.cin, self.cout, self.dtype = frag, ksize, cin, cout, dtype


def conv_planes_pack(weight):
    """weight [Cout,Cin,k,k] contiguous 16-bit -> PackedConvFilter (pvo_conv_planes_pack: once per parameter version, on the device)"""
    dev = _dev(weight)
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.dtype not in (torch.float16, torch.bfloat16) or not weight.is_contiguous():
        raise PvoHipError("conv_planes_pack: weight must be a contiguous 16-bit [Cout,Cin,k,k] tensor")
    Cout, Cin, k, _ = weight.shape
    lib = _lib.load()
    nbytes = lib.pvo_conv_planes_filter_bytes(k, Cin, Cout)
    if nbytes == 0:
        raise PvoHipError("conv_planes_pack: unsupported filter %d x %d, %d -> %d channels" % (k, k, Cin, Cout))
    frag = torch.empty(nbytes // 2, dtype=weight.dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.pvo_conv_planes_pack(_ptr(weight), _ptr(frag), k, Cin, Cout, _dtype_code(weight, "weight"), _stream(dev)), "conv_planes_pack")
    return PackedConvFilter(frag, k, Cin, Cout, weight.dtype)


def conv_planes(x, packed, bias=None, residual=None, stride=1, relu_inner=False, relu_outer=False, out=None):
    """Conv2d(Cin, Cout, k, stride, padding = k // 2) on a contiguous 16-bit NCHW tensor, deterministic, on the matrix cores
    (pvo_conv_planes), and what follows it in a norm-free encoder layer: relu_outer(residual + relu_inner(conv(x) + bias[c])), every step
    rounded to x's dtype as bias_norm_act(norm=False) rounds it.  x [N,Cin,H,W], packed = conv_planes_pack(weight), bias [Cout] or None,
    residual [N,Cout,Ho,Wo] or None -> [N,Cout,(H-1)//stride+1,(W-1)//stride+1] (`out`, if given; it must not be x)"""
    if not isinstance(packed, PackedConvFilter):
        raise PvoHipError("conv_planes: packed must come from conv_planes_pack")
    dev = _dev(x, packed.frag, bias, residual, out)
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16) or not x.is_contiguous():
        raise PvoHipError("conv_planes: x must be a contiguous 16-bit [N,Cin,H,W] tensor")
    N, Cin, H, W = x.shape
    stride = int(stride)
    if packed.dtype != x.dtype or packed.cin != Cin:
        raise PvoHipError("conv_planes: the packed filter is %s with %d input channels, x is %s with %d" % (packed.dtype, packed.cin, x.dtype, Cin))
    Cout, k = packed.cout, packed.ksize
    if stride < 1 or not conv_planes_supported(k, stride, Cin, Cout):
        raise PvoHipError("conv_planes: unsupported convolution %d x %d stride %d, %d -> %d channels" % (k, k, stride, Cin, Cout))
    shape = (N, Cout, (H - 1) // stride + 1 if H else 0, (W - 1) // stride + 1 if W else 0)
    for t, n in ((bias, "bias"), (residual, "residual"), (out, "out")):
        if t is not None and (t.dtype != x.dtype or not t.is_contiguous()):
            raise PvoHipError("conv_planes: %s must be contiguous and have x's dtype" % n)
    if bias is not None and bias.numel() != Cout or residual is not None and tuple(residual.shape) != shape \
            or out is not None and tuple(out.shape) != shape:
        raise PvoHipError("conv_planes: bias [Cout], residual and out of the result's shape %s" % (shape,))
    if out is not None and out.numel() and x.numel() and out.untyped_storage().data_ptr() == x.untyped_storage().data_ptr() \
            and out.data_ptr() < x.data_ptr() + x.numel() * 2 and x.data_ptr() < out.data_ptr() + out.numel() * 2:
        raise PvoHipError("conv_planes: out must not alias x")
    y = torch.empty(shape, dtype=x.dtype, device=dev) if out is None else out
    with torch.cuda.device(dev):
        check(_lib.load().pvo_conv_planes(_ptr(x), _ptr(packed.frag), _vp(bias), _vp(residual), _ptr(y), N, Cin, Cout, H, W, k, stride,
                                          1 if relu_inner else 0, 1 if relu_outer else 0, _dtype_code(x, "x"), _stream(dev)), "conv_planes")
    return y


_FRAME_KINDS = {torch.int32: 0, torch.uint8: 1, torch.float32: 2}


def frame_normalise(image, mean, std, dtype=torch.float16):
    """[3,H,W] BGR frame (int32 / uint8 / float32, 0..255) on the device -> [1,3,H,W] RGB `dtype`, ((v / 255) - mean) / std in fp32 then
    rounded (pvo_frame_normalise); mean / std: sequences of three Python floats"""
    dev = _dev(image)
    _contig(image, "image")
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype not in _FRAME_KINDS:
        raise PvoHipError("frame_normalise: a contiguous [3,H,W] int32 / uint8 / float32 frame")
    _, H, W = image.shape
    out = torch.empty(1, 3, H, W, dtype=dtype, device=dev)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean]); s = (ctypes.c_float * 3)(*[float(v) for v in std])
    with torch.cuda.device(dev):
        check(_lib.load().pvo_frame_normalise(_ptr(image), _ptr(out), H, W, m, s, _FRAME_KINDS[image.dtype], _DT[dtype], _stream(dev)), "frame_normalise")
    return out


def debug_config(knob, value):
    """the library's test hook (include/pvo_hip.h pvo_debug_config): "ba_solver" = None | "blocked" | "wave" | "pipe" | "twin" | "dense" | "blocks",
    "heads_gather_flat" = bool, "no_riders" = bool, "post_separate" = bool,
    "edge_blocks" = None | "off" | "half" | "third", with "+low" / "+agg" / "+trunk" (or the header's number).  Process-wide; tests that compare bit-identical forms call it in a process of
    their own.  (These were environment variables read inside the library until round 5.)"""
    knobs = {"ba_solver": _lib.PVO_KNOB_BA_SOLVER, "heads_gather_flat": _lib.PVO_KNOB_HEADS_GATHER_FLAT, "no_riders": _lib.PVO_KNOB_NO_RIDERS,
             "post_separate": _lib.PVO_KNOB_POST_SEPARATE, "edge_blocks": _lib.PVO_KNOB_EDGE_BLOCKS}
    if knob == "edge_blocks" and value is None:
        value = 0
    if knob == "edge_blocks" and isinstance(value, str) and not value.isdigit():
        # "off", or "half" | "third" (the leading block's share of the edges) with "+low" (the trailing block's stream of the lowest
        # priority), "+agg" (GraphAgg.conv1 per block too) and "+trunk" (the trunk per block too: each block's lookup and encoders in
        # front of its own gates) in any order: "third+low+agg+trunk"
        parts = value.split("+")
        if parts[0] == "off" and len(parts) == 1:
            value = 1
        else:
            if parts[0] not in ("half", "third") or any(p not in ("low", "agg", "trunk") for p in parts[1:]):
                raise ValueError("edge_blocks: " + value)
            value = 2 + (parts[0] == "third") + 2 * ("low" in parts[1:]) + 4 * ("agg" in parts[1:]) + 8 * ("trunk" in parts[1:])
    if knob == "ba_solver":
        value = {None: 0, "": 0, "blocked": 1, "wave": 2, "pipe": 3, "twin": 4, "dense": 5, "blocks": 6}[value]
    check(_lib.load().pvo_debug_config(knobs[knob], int(value)), "pvo_debug_config")


def graph_update_workspace(E, K, R, H, W, max_segments, device):
    n = _lib.load().pvo_graph_update_workspace_bytes(int(E), int(K), int(R), int(H), int(W), int(max_segments))
    return _op_workspace(("up", torch.device(device).index), torch.device(device), n)


def graph_update(weights, args, workspace, stereo_baseline=0.0, static_rows=None):
    """FactorGraph.update (factor_graph.py:227-307) as ONE call: `args` is a filled _lib.GraphUpdateArgs (the caller -
    pvo_amd.factor_graph - keeps every tensor it points to alive); see include/pvo_hip.h pvo_graph_update.
    stereo_baseline > 0 (pvo_graph_update_rig): edges (i, i) are stereo edges of a rectified rig with that baseline.
    static_rows (device int32 [E], pvo_graph_update_rows): args.op.P_zr / P_q are per-keyframe pools read at static_rows[e]."""
    dev = workspace.device
    stereo_baseline = _baseline(stereo_baseline, "graph_update")
    with torch.cuda.device(dev):
        if static_rows is not None:
            if static_rows.dtype != torch.int32 or static_rows.numel() != args.op.E or static_rows.device != dev:
                raise PvoHipError("graph_update: static_rows must be a device int32 [E] tensor")
            check(_lib.load().pvo_graph_update_rows(ctypes.byref(weights.struct), ctypes.byref(args), ctypes.c_void_p(workspace.data_ptr()),
                                                    workspace.numel(), stereo_baseline, _ptr(static_rows), _stream(dev)),
                  "graph_update (frame rows)")
        elif stereo_baseline == 0.0:
            check(_lib.load().pvo_graph_update(ctypes.byref(weights.struct), ctypes.byref(args), ctypes.c_void_p(workspace.data_ptr()),
                                               workspace.numel(), _stream(dev)), "graph_update")
        else:
            check(_lib.load().pvo_graph_update_rig(ctypes.byref(weights.struct), ctypes.byref(args), ctypes.c_void_p(workspace.data_ptr()),
                                                   workspace.numel(), stereo_baseline, _stream(dev)), "graph_update (stereo)")


# --------------------------------------------------------------------------- convex upsampling
def _cvx_mask_layout(mask, what):
    """mask [B,576,H,W]: planar (contiguous) -> 1, channels-last ([B,H,W,576] in memory, what the update operator writes) -> 0"""
    if mask.dim() != 4 or mask.shape[1] != 576:
        raise PvoHipError("%s: mask must be [B,576,H,W] (9 taps x 8 x 8 logits); got %s" % (what, tuple(mask.shape)))
    if mask.is_contiguous():
        return 1
    if mask.permute(0, 2, 3, 1).is_contiguous():
        return 0
    raise RuntimeError("mask must be contiguous")


def _cvx_rows(rows, B, n, dev, name):
    """a row table: None, a host sequence (range-checked here) or a device int64 tensor [B] (entries outside the buffer are no-ops)"""
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor):
        rows = [int(r) for r in rows]
        if any(r < 0 or r >= n for r in rows):
            raise PvoHipError("cvx_upsample: %s names a row outside the buffer of %d rows" % (name, n))
        rows = to_device_async(rows, torch.long, dev)
    _dev(rows); _long(rows, name); _contig(rows, name)
    if rows.dim() != 1 or rows.shape[0] != B:
        raise PvoHipError("cvx_upsample: %s must have one entry per mask row (%d)" % (name, B))
    return rows


def cvx_upsample(data, mask, out=None, in_rows=None, out_rows=None):
    """droid_net.cvx_upsample as ONE kernel (pvo_cvx_upsample): data [N,H,W,D] fp32 / fp64 with D = 1 or 2, mask [B,576,H,W] logits -
    contiguous (planar) or channels-last, fp16 / bf16 / fp32 with fp32 data, fp64 with fp64 data - -> out [N',8H,8W,D].
    in_rows / out_rows (int64 [B] on the device, or host sequences): mask row b reads data[in_rows[b]] and writes out[out_rows[b]];
    without them N = B and a fresh out has B rows.  Rows of `out` that no mask row names are not touched."""
    dev = _dev(data, mask, out)
    _contig(data, "data")
    planar = _cvx_mask_layout(mask, "cvx_upsample")
    if data.dim() != 4 or data.shape[3] not in (1, 2) or tuple(data.shape[1:3]) != tuple(mask.shape[2:]):
        raise PvoHipError("cvx_upsample: data must be [N,H,W,D] with D = 1 or 2 and the mask's H, W; got %s for mask %s"
                          % (tuple(data.shape), tuple(mask.shape)))
    B, _, H, W = mask.shape
    N, D = data.shape[0], data.shape[3]
    if out is None:
        out = torch.empty(B if out_rows is None else N, 8 * H, 8 * W, D, dtype=data.dtype, device=dev)
    _contig(out, "out")
    if out.dim() != 4 or tuple(out.shape[1:]) != (8 * H, 8 * W, D) or out.dtype != data.dtype:
        raise PvoHipError("cvx_upsample: out must be [N',%d,%d,%d] %s" % (8 * H, 8 * W, D, data.dtype))
    if (in_rows is None and N < B) or (out_rows is None and out.shape[0] < B):
        raise PvoHipError("cvx_upsample: %d mask rows need %d rows of data and out (or row tables)" % (B, B))
    in_rows = _cvx_rows(in_rows, B, N, dev, "in_rows")
    out_rows = _cvx_rows(out_rows, B, out.shape[0], dev, "out_rows")
    with torch.cuda.device(dev):
        check(_lib.load().pvo_cvx_upsample(_ptr(data), _ptr(mask), _ptr(out), _vp(in_rows), _vp(out_rows), N, out.shape[0], B, H, W, D,
                                           mask.shape[1], planar, _dtype_code(data, "cvx_upsample"), _dtype_code(mask, "cvx_upsample"),
                                           _stream(dev)), "cvx_upsample")
    return out


def cvx_upsample_vjp(data, mask, gout):
    """(gmask in the mask's layout, gdata) of cvx_upsample(data, mask) for the output gradient gout [B,8H,8W,D]; fp32 or fp64 throughout,
    bit-identical from call to call (pvo_cvx_upsample_vjp)"""
    dev = _dev(data, mask, gout)
    _contig(data, "data"); _contig(gout, "gout")
    planar = _cvx_mask_layout(mask, "cvx_upsample_vjp")
    B, _, H, W = mask.shape
    D = data.shape[-1]
    if tuple(data.shape) != (B, H, W, D) or tuple(gout.shape) != (B, 8 * H, 8 * W, D) or not (data.dtype == mask.dtype == gout.dtype) \
            or data.dtype not in (torch.float32, torch.float64):
        raise PvoHipError("cvx_upsample_vjp: data [B,H,W,D], mask [B,576,H,W], gout [B,8H,8W,D], all fp32 or all fp64")
    gmask, gdata = torch.empty_like(mask), torch.empty_like(data)         # (preserve_format: the mask's own layout)
    lib = _lib.load()
    dt = _DT[data.dtype]
    scratch = torch.empty(lib.pvo_cvx_upsample_vjp_scratch_bytes(B, H, W, D, dt), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.pvo_cvx_upsample_vjp(_ptr(data), _ptr(mask), _ptr(gout), _ptr(gmask), _ptr(gdata), B, H, W, D, mask.shape[1], planar, dt,
                                       _ptr(scratch), scratch.numel(), _stream(dev)), "cvx_upsample_vjp")
    return gmask, gdata


# --------------------------------------------------------------------------- SE3 element-wise operations
SE3_OPS = {"exp": 0, "log": 1, "inv": 2, "mul": 3, "act4": 4, "act3": 5, "adj": 6, "adjT": 7}
_SE3_OUT = {"exp": 7, "log": 6, "inv": 7, "mul": 7, "act4": 4, "act3": 3, "adj": 6, "adjT": 6}


def se3_unary(op, x):
    """exp [n,6] -> [n,7], log [n,7] -> [n,6], inv [n,7] -> [n,7] (lietorch SE3, forward); x contiguous f32 / f64"""
    dev = _dev(x)
    _contig(x, "x")
    if x.dtype not in (torch.float32, torch.float64):
        raise PvoHipError("se3: float32 / float64 only")
    n = x.numel() // x.shape[-1]
    y = torch.empty(x.shape[:-1] + (_SE3_OUT[op],), dtype=x.dtype, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_se3_unary(SE3_OPS[op], _ptr(x), _ptr(y), n, _DT[x.dtype], _stream(dev)), "se3_" + op)
    return y


def se3_binary(op, a, rep_a, b, rep_b, out_batch):
    """mul / act4 / act3 / adj / adjT with index broadcasting: output element i reads a[i // rep_a], b[i // rep_b]"""
    dev = _dev(a, b)
    _contig(a, "a"); _contig(b, "b")
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.float64):
        raise PvoHipError("se3: both operands float32 or both float64")
    y = torch.empty(tuple(out_batch) + (_SE3_OUT[op],), dtype=a.dtype, device=dev)
    n = y.numel() // _SE3_OUT[op]
    with torch.cuda.device(dev):
        check(_lib.load().pvo_se3_binary(SE3_OPS[op], _ptr(a), int(rep_a), _ptr(b), int(rep_b), _ptr(y), n, _DT[a.dtype],
                                         _stream(dev)), "se3_" + op)
    return y


def se3_unary_vjp(op, x, gy):
    """gx of se3_unary(op, x) for the output gradient gy (ambient coordinates)"""
    dev = _dev(x, gy)
    _contig(x, "x"); _contig(gy, "gy")
    n = x.numel() // x.shape[-1]
    gx = torch.empty_like(x)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_se3_unary_vjp(SE3_OPS[op], _ptr(x), _ptr(gy), _ptr(gx), n, _DT[x.dtype], _stream(dev)), "se3_%s_vjp" % op)
    return gx


def se3_binary_vjp(op, a, rep_a, b, rep_b, gy, need_a=True, need_b=True):
    """(ga, gb) of se3_binary for the output gradient gy, summed over the repeats of a broadcast operand"""
    dev = _dev(a, b, gy)
    _contig(a, "a"); _contig(b, "b"); _contig(gy, "gy")
    nb = _SE3_OUT[op]
    n = gy.numel() // nb
    ga = torch.empty((n, 7), dtype=a.dtype, device=dev) if need_a else None
    gb = torch.empty((n, nb), dtype=a.dtype, device=dev) if need_b else None
    with torch.cuda.device(dev):
        check(_lib.load().pvo_se3_binary_vjp(SE3_OPS[op], _ptr(a), int(rep_a), _ptr(b), int(rep_b), _ptr(gy), _vp(ga), _vp(gb), n,
                                             _DT[a.dtype], _stream(dev)), "se3_%s_vjp" % op)
    if ga is not None:
        ga = (ga.view(-1, int(rep_a), 7).sum(1) if rep_a > 1 else ga).view(a.shape)
    if gb is not None:
        gb = (gb.view(-1, int(rep_b), nb).sum(1) if rep_b > 1 else gb).view(b.shape)
    return ga, gb


def proj_transform(poses, depths, intrinsics, ii, jj, jacobian=False, return_depth=False):
    """projective_ops.projective_transform as ONE kernel (pvo_proj_transform): poses [B,P,7], depths [B,P,H,W], intrinsics [B,P,4]
    (fp32 or fp64, one device), ii / jj int64 [N] on that device -> coords [B,N,H,W,2|3], valid [B,N,H,W,1] and, with
    `jacobian`, (Ji [B,N,H,W,2,6], Jj [B,N,H,W,2,6], Jz [B,N,H,W,2,1])"""
    dev = _dev(poses, depths, intrinsics, ii, jj)
    for t, n in ((poses, "poses"), (depths, "depths"), (intrinsics, "intrinsics"), (ii, "ii"), (jj, "jj")):
        _contig(t, n)
    _long(ii, "ii"); _long(jj, "jj")
    B, P, ht, wd = depths.shape
    N, nx = ii.shape[0], 3 if return_depth else 2
    if poses.shape != (B, P, 7) or intrinsics.shape != (B, P, 4) or poses.dtype != depths.dtype or intrinsics.dtype != depths.dtype:
        raise PvoHipError("proj_transform: poses [B,P,7], depths [B,P,H,W], intrinsics [B,P,4] of one dtype")
    new = lambda *sh: torch.empty(sh, dtype=depths.dtype, device=dev)
    x1, valid = new(B, N, ht, wd, nx), new(B, N, ht, wd, 1)
    Ji, Jj, Jz = (new(B, N, ht, wd, 2, 6), new(B, N, ht, wd, 2, 6), new(B, N, ht, wd, 2, 1)) if jacobian else (None, None, None)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_proj_transform(_ptr(poses), _ptr(depths), _ptr(intrinsics), _ptr(ii), _ptr(jj), B, P, N, ht, wd, nx,
                                             _ptr(x1), _ptr(valid), _vp(Ji), _vp(Jj), _vp(Jz), _DT[depths.dtype], _stream(dev)), "proj_transform")
    return (x1, valid, (Ji, Jj, Jz)) if jacobian else (x1, valid)


def proj_transform_vjp(poses, depths, intrinsics, ii, jj, g_x1, g_Ji, g_Jj, g_Jz):
    """gradients of proj_transform's outputs (any may be None) -> (grad poses [B,P,7], grad depths [B,P,H,W]), ambient coordinates"""
    dev = _dev(poses, depths, intrinsics, ii, jj)
    B, P, ht, wd = depths.shape
    gs = [None if g is None else g.contiguous() for g in (g_x1, g_Ji, g_Jj, g_Jz)]
    nx = gs[0].shape[-1] if gs[0] is not None else 2
    gp, gd = torch.zeros_like(poses), torch.zeros_like(depths)
    with torch.cuda.device(dev):
        check(_lib.load().pvo_proj_transform_vjp(_ptr(poses), _ptr(depths), _ptr(intrinsics), _ptr(ii), _ptr(jj), B, P, ii.shape[0], ht, wd, nx,
                                                 _vp(gs[0]), _vp(gs[1]), _vp(gs[2]), _vp(gs[3]), _ptr(gp), _ptr(gd), _DT[depths.dtype], _stream(dev)),
              "proj_transform_vjp")
    return gp, gd


def _check_ba_plan(plan, N, P):
    """the plan of ba_train (ba_native.make_plan): four contiguous int32 vectors kx [M], kk [N], kptr [M+1], kedge [N], 1 <= M <= P.
    Returns M.  (Whether it was built from this ii is not checked: that would read the device.)"""
    if len(plan) != 4 or any(not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() for t in plan):
        raise PvoHipError("ba_train: the plan is four contiguous int32 vectors (kx, kk, kptr, kedge), as ba_native.make_plan builds it")
    kx, kk, kptr, kedge = plan
    M = kx.shape[0]
    if not 1 <= M <= P or kk.shape[0] != N or kedge.shape[0] != N or kptr.shape[0] != M + 1:
        raise PvoHipError("ba_train: plan of %d keyframes with kk [%d], kptr [%d], kedge [%d] does not fit %d edges over %d frames"
                          % (M, kk.shape[0], kptr.shape[0], kedge.shape[0], N, P))
    return M


def ba_train(poses, disps, intrinsics, target, weight, eta, ii, jj, plan, fixedp):
    """one Gauss-Newton step of geom.ba.BA (pvo_ba_train): poses [B,P,7], disps [B,P,H,W], intrinsics [B,P,4], target / weight
    [B,N,H,W,2], eta [B,M,H,W] of one dtype (fp32 / fp64) on one device; ii / jj int64 [N] and the plan (kx, kk, kptr, kedge: int32)
    there too -> (poses [B,P,7], disps [B,P,H,W], dx [B,6(P-fixedp)], workspace).  The workspace holds the state pvo_ba_train_vjp reads:
    keep it with the call until its backward"""
    dev = _dev(poses, disps, intrinsics, target, weight, eta, ii, jj, *plan)
    for t, n in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (target, "target"), (weight, "weight"), (eta, "eta"),
                 (ii, "ii"), (jj, "jj")):
        _contig(t, n)
    _long(ii, "ii"); _long(jj, "jj")
    B, P, ht, wd = disps.shape
    N, M = ii.shape[0], _check_ba_plan(plan, ii.shape[0], P)
    if (poses.shape != (B, P, 7) or intrinsics.shape != (B, P, 4) or target.shape != (B, N, ht, wd, 2) or weight.shape != target.shape
            or eta.numel() != B * M * ht * wd or len({t.dtype for t in (poses, disps, intrinsics, target, weight, eta)}) != 1):
        raise PvoHipError("ba_train: poses [B,P,7], disps [B,P,H,W], intrinsics [B,P,4], target / weight [B,N,H,W,2], eta [B,M,H,W] of one dtype")
    dt = _DT[disps.dtype]
    lib = _lib.load()
    ws = torch.empty(lib.pvo_ba_train_workspace_bytes(B, P, N, M, ht * wd, dt), dtype=torch.uint8, device=dev)
    pout, dout = torch.empty_like(poses), torch.empty_like(disps)
    dx = torch.empty(B, 6 * (P - fixedp), dtype=disps.dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.pvo_ba_train(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(target), _ptr(weight), _ptr(eta), _ptr(ii), _ptr(jj),
                               *[_ptr(t) for t in plan], B, P, N, M, ht, wd, fixedp, _ptr(pout), _ptr(dout), _ptr(dx),
                               _ptr(ws), ws.numel(), dt, _stream(dev)), "ba_train")
    return pout, dout, dx, ws


def ba_train_vjp(poses, disps, intrinsics, target, weight, ii, jj, plan, fixedp, ws, g_poses, g_disps):
    """gradients of ba_train's poses / disps (the forward's inputs and workspace) -> (grad target, weight, eta [B,M,H,W], poses, disps);
    the backward's scratch is allocated here and released with the call"""
    dev = _dev(poses, disps, intrinsics, target, weight, ii, jj, ws, g_poses, g_disps, *plan)
    g_poses, g_disps = g_poses.contiguous(), g_disps.contiguous()
    B, P, ht, wd = disps.shape
    N, M = ii.shape[0], _check_ba_plan(plan, ii.shape[0], P)
    lib = _lib.load()
    scratch = torch.empty(lib.pvo_ba_train_vjp_scratch_bytes(B, P, N, M, ht * wd, _DT[disps.dtype]), dtype=torch.uint8, device=dev)
    gt, gw = torch.empty_like(target), torch.empty_like(weight)
    ge = torch.empty(B, M, ht, wd, dtype=disps.dtype, device=dev)
    gp, gd = torch.empty_like(poses), torch.empty_like(disps)
    with torch.cuda.device(dev):
        check(lib.pvo_ba_train_vjp(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(target), _ptr(weight), _ptr(ii), _ptr(jj),
                                   *[_ptr(t) for t in plan], B, P, N, M, ht, wd, fixedp, _ptr(g_poses), _ptr(g_disps),
                                   _ptr(gt), _ptr(gw), _ptr(ge), _ptr(gp), _ptr(gd), _ptr(ws), ws.numel(), _ptr(scratch), scratch.numel(),
                                   _DT[disps.dtype], _stream(dev)), "ba_train_vjp")
    return gt, gw, ge, gp, gd


STAGES = {"lookup": 0, "gates": 1, "candidate": 2, "ba": 3, "update": 4, "empty": 5}


_side_streams = {}


def side_stream(device):
    """the library's own second stream on `device` (pvo_side_stream) as a torch stream: work that is only needed by the
    next update can be queued beside the launch stream without creating another HIP stream"""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _side_streams.get(idx)
    if st is None:
        out = ctypes.c_void_p()
        with torch.cuda.device(idx):
            check(_lib.load().pvo_side_stream(ctypes.byref(out)), "side_stream")
        st = _side_streams[idx] = torch.cuda.ExternalStream(out.value, device=torch.device("cuda", idx))
    return st


_upload_streams = {}


def upload_stream(device):
    """ONE stream per device for asynchronous host-to-device frame uploads (the pipelined tracker), created once per process behind the
    library's second stream.  The runtime hands a new stream the hardware queue with the fewest streams on it at that moment: a stream
    created per tracker landed on a different queue in every tracker of a process - the first pipelined pass of bench.py's sequence leg
    ran at 147 frames/s, the next two at 103 and 106 with their upload stream on a queue the operator's kernels were using."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _upload_streams.get(idx)
    if st is None:
        side_stream(device)
        st = _upload_streams[idx] = torch.cuda.Stream(torch.device("cuda", idx))
    return st


def clock_probe(stream, iters=20000):
    """launch the shader-clock probe on `stream` (a torch.cuda.Stream); returns the device tensor it fills - after a
    synchronize, `clock_ghz(t)` is the clock the chip held while the probe ran"""
    dev = torch.device("cuda", stream.device_index if hasattr(stream, "device_index") else torch.cuda.current_device())
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        # (allocated ON `stream`: a block the caching allocator recycles for the current stream may still be in use by
        # kernels queued there, which is only safe for work ordered behind them)
        out = torch.zeros(3, dtype=torch.int64, device=dev)
        check(_lib.load_probe().pvo_clock_probe(_ptr(out), int(iters), ctypes.c_void_p(stream.cuda_stream)), "clock_probe")
    return out


def mem_probe_gbps(device, nbytes=1 << 30, iters=16, blocks=8192, reps=5):
    """GB/s of fetched lines for consecutive 128-byte lines, random 128-byte lines and random 64-byte half lines
    (pvo_mem_probe; HIP events on the current stream): what this part's memory system sustains for scattered lines"""
    dev = torch.device(device)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    lib, out = _lib.load_probe(), {}
    with torch.cuda.device(dev):
        for name, mode in (("streaming_128B", 0), ("random_128B", 1), ("random_64B", 2)):
            run = lambda: lib.pvo_mem_probe(_ptr(buf), nbytes, mode, iters, blocks, _ptr(sink), _stream(dev))
            for _ in range(2):
                fetched = run()
            if fetched < 0:
                raise PvoHipError("mem_probe failed")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record(); torch.cuda.synchronize(dev)
            out[name] = fetched / (e0.elapsed_time(e1) / reps) / 1e6
    return out


def clock_ghz(t):
    c, r, _ = t.tolist()
    return c / (r * 10.0) if r else float("nan")


def probe_arm(stage, capacity, every=1):
    """record HIP events around `stage` ("lookup" | "gates" | "candidate" | "ba" | "update") of the next native updates,
    one occurrence in `every`"""
    check(_lib.load().pvo_probe_arm_every(STAGES[stage], int(capacity), int(every)), "probe_arm")


def probe_read(capacity):
    """elapsed milliseconds of the recorded stage occurrences (waits for them); disarms the probe"""
    buf = (ctypes.c_float * int(capacity))()
    n = _lib.load().pvo_probe_read(buf, int(capacity))
    if n < 0:
        raise PvoHipError("probe_read failed")
    return [float(buf[i]) for i in range(n)]
