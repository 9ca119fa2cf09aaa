"""HIP-graph replay of fixed-shape per-frame work (the encoders of MotionFilter / PoseTrajectoryFiller).

The reference issues its per-frame encoders (VO_Module/droid_slam/motion_filter.py:52-60, trajectory_filler.py:32-38) as ~70 eager
PyTorch / cuDNN launches per network.  On the sequence run of bench.py that is 4.6 ms of HOST time per network call for ~0.3 ms of
device work: the device idles 73 % of a tracked sequence.  `GraphedCall` captures such a callable once per input signature into a HIP
graph (torch.cuda.CUDAGraph = hipGraph on ROCm) and replays it with one launch; the inputs are copied into the capture's static
buffers, the outputs are the capture's static buffers (a caller that keeps one across calls clones it).

Safe by construction: the first `warmup` calls run eagerly (MIOpen picks its kernels there), the first replay is compared with
an eager run of the same input, and any failure - capture not supported, mismatch - switches the instance back to eager for good.
`pvo_amd.config.debug_config("hip_graphs", False)` disables capture process-wide (nothing is read from the environment).
"""
import gc

import torch

from . import config


def _version(t):
    try:
        return t._version
    except RuntimeError:                        # (inference tensors carry no version counter: always copied)
        return None


def _flat(out):
    return (out,) if isinstance(out, torch.Tensor) else tuple(out)


class GraphedCall:
    def __init__(self, fn, warmup=2, rtol=2e-3, name=None, guard=None, frozen=()):
        """fn(*tensors) -> tensor or tuple of tensors; no host synchronisation and no data-dependent shapes inside.
        guard() (optional) -> a hashable that must be unchanged for a capture to stay valid (e.g. the storage of the weights).
        frozen: which arguments the CALLER declares immutable for as long as it keeps passing the same tensor object - a set of
        positions, or a callable position -> bool.  Only those may skip the copy into the capture's static buffer when they are the
        same object with an unchanged version counter as at the previous replay.  Every other argument is copied on every call: a
        version counter says nothing about tensors this library's kernels write through data_ptr(), so the skip is
        the caller's explicit promise, never inferred.  `config.debug_config("graph_check_skipped", True)` compares every skipped
        argument with the static buffer (a device synchronisation per call) and raises on a difference."""
        self.fn, self.warmup, self.rtol, self.name = fn, warmup, rtol, name or getattr(fn, "__name__", "call")
        self.guard = guard
        self.frozen = frozen if callable(frozen) else (lambda i, _s=frozenset(frozen): i in _s)
        self.cache = {}
        self.disabled = False
        self.replays = 0
        self.copies = self.skipped = 0

    def _key(self, args):
        return tuple((tuple(a.shape), a.dtype, a.device, a.stride()) for a in args) + ((self.guard(),) if self.guard else ())

    def __call__(self, *args):
        if self.disabled or not config.get("hip_graphs") or not args or not all(isinstance(a, torch.Tensor) and a.is_cuda for a in args) or torch.is_grad_enabled():
            return self.fn(*args)
        key = self._key(args)
        st = self.cache.get(key)
        if st is None:
            if len(self.cache) >= 4:            # (a guard that keeps changing: do not pile up captures)
                self.cache.clear()
            st = self.cache[key] = {"n": 0, "graph": None}
        if st["graph"] is None:
            if st["n"] < self.warmup:
                st["n"] += 1
                return self.fn(*args)
            try:
                self._capture(st, args)
            except Exception as e:              # capture unsupported for something inside fn: stay eager
                self.disabled = True
                self.error = repr(e)
                torch.cuda.synchronize()
                return self.fn(*args)
            if self.disabled:
                return self.fn(*args)
        # an argument the caller declared FROZEN that is the same tensor object as at the previous replay (version counter unchanged)
        # is already in the capture's static buffer: the motion filter hands its reference keyframe's maps - five to seven tensors -
        # to every frame's replay, and each device-to-device blit is ~48 us of host time in front of the launch (bench.py `sequence`).
        # (Identity, not address: the previous argument is kept alive here, so no new tensor can take its place in memory.)
        held = st["held"]
        dst, src = [], []
        check = config.get("graph_check_skipped")
        for i, (s, a) in enumerate(zip(st["in"], args)):
            h = held[i]
            ver = _version(a) if self.frozen(i) else None
            if h is not None and h[0] is a and ver is not None and h[1] == ver:
                if check and not torch.equal(s, a):
                    raise RuntimeError("GraphedCall %s: argument %d was declared frozen, was not copied, and differs from the capture's buffer" % (self.name, i))
                self.skipped += 1
                continue
            dst.append(s); src.append(a)
            held[i] = (a, ver)
        self.copies += len(dst)
        if len(dst) == 1:
            dst[0].copy_(src[0])
        elif dst:
            torch._foreach_copy_(dst, src)
        st["graph"].replay()
        self.replays += 1
        return st["out"] if st["single"] else tuple(st["outs"])

    def _capture(self, st, args):
        static_in = [torch.empty_like(a).copy_(a) for a in args]
        want = _flat(self.fn(*static_in))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        # No cyclic collection may run INSIDE the capture.  A GraphedCall and its owner refer to each other (fn is the owner's bound
        # method), so a dropped MotionFilter - with its captured graphs and their private memory pool - is freed by the cycle collector
        # whenever that next runs; when it ran between capture_begin and capture_end, releasing an older graph's memory is a call the
        # capturing stream does not permit, the error is raised in a destructor and the process aborts.  torch.cuda.graph used to collect
        # before every capture and no longer does (unless torch.compiler.config.force_cudagraph_gc), so: collect here, while nothing
        # is capturing, and keep the collector off until the capture has ended.
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                out = self.fn(*static_in)
        finally:
            if collecting:
                gc.enable()
        outs = _flat(out)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, want):
            scale = float(b.float().abs().max()) + 1e-12
            if a.shape != b.shape or not bool(torch.isfinite(a.float()).all()) == bool(torch.isfinite(b.float()).all()) or \
                    float((a.float() - b.float()).abs().max()) > self.rtol * scale:
                self.disabled = True
                self.error = "replay differs from the eager run"
                return
        st.update(graph=g, out=out, outs=outs, single=isinstance(out, torch.Tensor))
        st["in"] = static_in
        st["held"] = [None] * len(static_in)
