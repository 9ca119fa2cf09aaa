"""The encoders with `native_convs` (every 3 x 3 / 7 x 7 convolution on pvo_conv_planes instead of the vendor library): the whole
network against the module's own forward and against the reference's fixture, no vendor kernel and no process-global flag, captured
graphs across parameter updates, and a tracked sequence that repeats bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "droidnet_forward.npz")
ENCODERS = [("instance", 128), ("none", 256)]


def _encoder(norm_fn, out_dim, cuda, seed=3, native=True):
    from pvo_amd.modules.extractor import BasicEncoder
    torch.manual_seed(seed)
    enc = BasicEncoder(output_dim=out_dim, norm_fn=norm_fn).to(cuda).eval().half()
    enc.native_convs = native
    return enc


@pytest.mark.parametrize("norm_fn,out_dim", ENCODERS)
def test_native_encoder_equals_the_module_under_autocast(cuda, norm_fn, out_dim):
    """the bound tests/test_encoder_fused.py holds the vendor-convolution path to: max |diff| <= 2e-2 max |want|"""
    enc = _encoder(norm_fn, out_dim, cuda)
    g = torch.Generator().manual_seed(5)
    for (h, w) in ((240, 808), (64, 96)):
        x = torch.randn(1, 1, 3, h, w, generator=g).to(cuda)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            want = enc(x)
            got = enc.forward_inference(x)
        assert got.shape == want.shape and got.dtype == want.dtype
        scale = float(want.float().abs().max())
        err = float((got.float() - want.float()).abs().max())
        print(norm_fn, (h, w), "native: max |diff| %.3g of scale %.3g" % (err, scale))
        assert err <= 2e-2 * scale


def test_native_encoder_against_the_reference_fixture(cuda):
    """tests/golden/droidnet_forward.npz: the reference's BasicEncoder, seed 0 (identical weights by construction), fp32.  The native
    path's max error against it must be <= 2 x that of today's vendor-convolution forward_inference on the same weights: both are 13
    layers of fp16 roundings in two summation orders, the factor covers that spread on 4 x 6 planes."""
    from pvo_amd.modules.extractor import BasicEncoder
    z = np.load(GOLD)
    x = torch.from_numpy(z["enc_x"]).to(cuda)
    for norm_fn, od in ENCODERS:
        torch.manual_seed(0)
        enc = BasicEncoder(output_dim=od, norm_fn=norm_fn).eval().to(cuda).half()
        want = torch.from_numpy(z["enc_%s" % norm_fn]).to(cuda)
        errs = {}
        for native in (False, True):
            enc.native_convs = native
            with torch.no_grad():
                got = enc.forward_inference(x)
            assert got.shape == want.shape
            errs[native] = float((got.float() - want).abs().max())
        print(norm_fn, "max error against the reference fixture: native %.4g, vendor convolutions %.4g (scale %.3g)"
              % (errs[True], errs[False], float(want.abs().max())))
        assert errs[True] <= 2.0 * errs[False]


@pytest.mark.parametrize("norm_fn,out_dim", ENCODERS)
def test_no_vendor_kernel_and_no_global_flag(cuda, monkeypatch, norm_fn, out_dim):
    from pvo_amd import droid_backends as db
    enc = _encoder(norm_fn, out_dim, cuda)
    x = torch.randn(1, 2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).to(cuda)
    with torch.no_grad():
        want = enc.forward_inference(x).clone()

    def boom(*a, **k):
        raise AssertionError("a vendor convolution was called")
    monkeypatch.setattr(torch.nn.functional, "conv2d", boom)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    before = torch.backends.cudnn.deterministic
    assert before is False and enc.deterministic is True                      # (the vendor path would set the flag for the call)
    seen, real = [], db.conv_planes

    def spy(*a, **k):
        seen.append(torch.backends.cudnn.deterministic)
        assert torch.backends.cudnn.deterministic is before
        return real(*a, **k)
    monkeypatch.setattr(db, "conv_planes", spy)
    with torch.no_grad():
        got = enc.forward_inference(x)
    assert torch.backends.cudnn.deterministic is before
    assert len(seen) == 13 and not any(seen)                                   # the stem and twelve 3 x 3 layers
    assert torch.equal(got, want)
    enc.native_convs = False                                                   # the switch really selects
    with torch.no_grad(), pytest.raises(AssertionError, match="vendor convolution"):
        enc.forward_inference(x)
    assert torch.backends.cudnn.deterministic is before


def test_unsupported_layer_falls_back_for_that_layer_only(cuda):
    """a custom output_dim the 1 x 1 head kernel does not take: the head keeps the vendor path (and the flag handling), the stem and the twelve
    3 x 3 convolutions are native"""
    from pvo_amd import droid_backends as db
    enc = _encoder("none", 96, cuda)
    x = torch.randn(1, 1, 3, 64, 96, generator=torch.Generator().manual_seed(2)).to(cuda)
    calls, real = [], db.conv_planes
    db.conv_planes = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            got, want = enc.forward_inference(x), enc(x)
    finally:
        db.conv_planes = real
    assert len(calls) == 13 and not enc._all_native(db)
    assert float((got.float() - want.float()).abs().max()) <= 2e-2 * float(want.float().abs().max())


def _frames(n, ht, wd, seed=3):
    g = torch.Generator().manual_seed(seed)
    big = torch.randint(0, 256, (3, ht + 64, wd + 8 * n + 64), generator=g).float()
    big = torch.nn.functional.avg_pool2d(big[None], 5, stride=1, padding=2)[0]
    return [big[:, 16:16 + ht, 8 * t:8 * t + wd].round().int().contiguous() for t in range(n)]


def test_graphs_replay_the_native_encoders_across_parameter_updates(cuda):
    """MotionFilter's captured encoder graphs with native convolutions: a replay equals the eager call bit for bit, three replays are
    identical, and after an in-place load_state_dict the next calls compute with the NEW weights (the packed filters a capture has baked
    in are rebuilt, and the graph guard re-captures: BasicEncoder._native_filter)."""
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.droid_net import DroidNet
    from pvo_amd.motion_filter import MotionFilter
    ht, wd = 128, 160
    torch.manual_seed(0)
    net = DroidNet().to(cuda).eval()
    net.update.half(); net.fnet.half(); net.cnet.half()
    net.fnet.native_convs = net.cnet.native_convs = True
    others = []
    for seed in (1, 2):                                                        # different weights for each of the two updates below
        torch.manual_seed(seed)
        others.append(DroidNet().to(cuda).eval().half())
    mf = MotionFilter(net, DepthVideo((ht, wd), buffer=16, device=cuda), thresh=0.0, device=cuda)
    imgs = [f.to(cuda) for f in _frames(4, ht, wd)]
    with torch.no_grad():
        for graph, eager, other in ((mf._features_g, mf._features_dev, others[0]), (mf._context_g, mf._context_dev, others[1])):
            flat = lambda r: [t.clone() for t in ((r,) if isinstance(r, torch.Tensor) else r)]
            for phase in range(2):
                n0 = graph.replays
                for k in range(8):                                            # warm-up calls, the capture, then replays
                    got = flat(graph(imgs[k % 4]))
                    want = flat(eager(imgs[k % 4]))
                    assert all(torch.equal(a, b) for a, b in zip(got, want)), (graph.name, phase, k)
                assert graph.replays >= n0 + 4 and not graph.disabled, (graph.name, getattr(graph, "error", None))
                reps = [flat(graph(imgs[0])) for _ in range(3)]
                assert all(torch.equal(a, b) for r in reps[1:] for a, b in zip(reps[0], r))
                if phase == 0:
                    old = reps[0]
                    net.fnet.load_state_dict(other.fnet.state_dict())          # in place: same storage, new values, new version counters
                    net.cnet.load_state_dict(other.cnet.state_dict())
                    got = flat(graph(imgs[0]))                                 # the very next call
                    want = flat(eager(imgs[0]))
                    assert all(torch.equal(a, b) for a, b in zip(got, want))
                    assert not torch.equal(got[0], old[0])
                    other_way = [flat(eager(imgs[0]))]
                    net.fnet.load_state_dict(other.fnet.state_dict())          # (same values again: the version counters move all the same)
                    net.cnet.load_state_dict(other.cnet.state_dict())
                    assert all(torch.equal(a, b) for a, b in zip(flat(graph(imgs[0])), other_way[0]))
        # the whole tracked frame as one graph, through the public call
        for t, f in enumerate(_frames(8, ht, wd, seed=4)):
            mf.track(t, f, intrinsics=torch.tensor([wd * 0.8, wd * 0.8, wd / 2.0, ht / 2.0]))
        assert mf._frame_g.replays >= 3 and not mf._frame_g.disabled
        assert bool(torch.isfinite(mf.video.fmaps[:mf.video.counter].float()).all())


def test_sequence_with_native_encoders_repeats_bit_for_bit(cuda):
    """the 240 x 808 synthetic stream with segments and removals of tests/test_vo_system.py's graphs-against-eager test (44 frames),
    Droid(args.native_encoders = True), run twice: keyframe time stamps, poses, depths and the filled trajectory (PoseTrajectoryFiller:
    16-frame batches through fnet.forward_inference) are identical bit for bit, and finite.  (NOT compared with the vendor-path
    trajectory: with random-init weights the system is chaotic, such a comparison would measure only that.)"""
    import random
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.synthetic import drifting_texture_stream
    n = 44
    frames = list(drifting_texture_stream(n, seed=0))
    rng = random.Random(77)
    sched = [rng.random() < 0.25 for _ in range(4 * n)]
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        droid = Droid(default_args(device=str(cuda), image_size=[240, 808], buffer=64, segm_filter=True, thresh=0.8,
                                   filter_thresh=0.0, keyframe_thresh=0.0, native_encoders=True))
        assert droid.net.fnet.native_convs and droid.net.cnet.native_convs
        droid.frontend.keyframe_decision = lambda k, dist: sched[k]
        for t, image, intr, segm in frames:
            droid.track(t, image, intrinsics=intr, segments=segm)
        kf = int(droid.video.counter)
        res = dict(kept=droid.video.tstamp[:kf].cpu().clone(), poses=droid.video.poses[:kf].cpu().clone(),
                   disps=droid.video.disps[:kf].cpu().clone(), replays=droid.filterx._frame_g.replays)
        res["traj"] = torch.from_numpy(droid.terminate(iter(frames), need_inv=True)).clone()
        runs.append(res)
        del droid
    a, b = runs
    assert a["replays"] >= n // 2 and 20 <= a["kept"].shape[0] < n and a["traj"].shape == (n, 7)
    for key in ("kept", "poses", "disps", "traj"):
        assert bool(torch.isfinite(a[key].float()).all()), key
        assert torch.equal(a[key], b[key]), key


def test_default_is_off():
    from pvo_amd.droid import default_args
    from pvo_amd.modules.extractor import BasicEncoder
    assert BasicEncoder.native_convs is False and not getattr(default_args(), "native_encoders", False)
