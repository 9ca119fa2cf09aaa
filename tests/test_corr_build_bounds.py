"""The correlation volume build (pvo_amd/csrc/corr_build.hip) against the fp64 contract of corr_build_reference.py: level 0 within a
bound built from the number formats and the channel count alone, every pooled level EQUAL to the exact pooling of the stored level
below, every level bit for bit on small-integer features, outputs and inputs between guards - at every epilogue of the matrix-core
kernel (aligned row-major, ragged, tiled), every call form (num_levels 1..4, out_slots, frame rows, misaligned level and feature
pointers), the generic path in all four types and both layouts, the refusals of the three C entry points, and CorrVolumePool
(row-major 16-bit, growth, fp32).  No element is exempt from a bound and no bound is tuned.

The GPU tests carry the gpu mark one by one, because the module also holds the CPU tests which prove that the checks fail on a
stand-in that truncates, drops a product, swaps two channels, transposes the pixels, reads a wrong edge, pools the unrounded level
or shifts the pooling window - and that the tolerance of tests/test_corr_build.py accepts the truncating one.

Largest err / bound observed on an MI355X (printed by every level-0 test; asserted only to be <= 1):
  matrix-core row-major 0.995 (C = 16, 8x64, bf16)    tiled 0.995 (C = 16, 8x64, bf16; the same through frame rows)
  generic fp32 0.495    generic fp64 0.0786    generic on 16-bit operands 0.990 (fp16), 0.988 (bf16)
(the 16-bit figures are the rounding to storage itself: u |ref| is nearly all of the bound, and a value that falls halfway between two
stored numbers uses all of it; the CPU stand-in reaches 0.992 on its cases)."""
import ctypes
import functools

import pytest
import torch

import corr_build_reference as R
import operator_bounds_util as B

gpu = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
N = 2


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


def _seed(*v):
    s = 29
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31)
    return s


@functools.lru_cache(maxsize=None)
def _features(C, H, W, dtype, integer, n=N):
    """shared by every test of a shape, never modified"""
    return R.features(_seed(C, H, W, integer), n, H, W, C, dtype, integer)


# ------------------------------------------------------------------------------------------------ CPU: the checks can fail
def _cpu_cases():
    return [(c, dt) for c in R.CPU_CASES for dt in DTYPES]


@pytest.mark.parametrize("case,dtype", _cpu_cases(), ids=_id)
def test_checks_pass_the_clean_standin_and_reject_every_mutation(case, dtype):
    C, H, W = case
    f1, f2 = _features(C, H, W, dtype, False)
    clean = R.standin_build(f1, f2, dtype)
    R.check_shapes(clean, N, H, W)
    assert R.check_level0(clean[0], f1, f2, "clean stand-in %s %s" % (case, dtype)) < 1.0
    R.check_pooled(clean, "clean stand-in")
    for m in R.LEVEL0_MUTATIONS:
        with pytest.raises(AssertionError, match="over the bound"):
            R.check_level0(R.standin_build(f1, f2, dtype, mutation=m)[0], f1, f2, m)
    for m in R.POOL_MUTATIONS:
        lv = R.standin_build(f1, f2, dtype, mutation=m)
        assert R.check_level0(lv[0], f1, f2, m) < 1.0                        # level 0 is clean: only the equality can see these
        with pytest.raises(AssertionError, match="elements differ"):
            R.check_pooled(lv, m)


def test_old_tolerance_accepts_truncated_rounding():
    """the gap this module closes: level 0 rounded toward zero instead of to nearest errs by up to 2 u |ref|.  The assertion of
    test_mfma_build_matches_oracle_and_pools_exactly (1.01 * 2 u * |ref| + 1e-4) accepts it on all eight cases; the derived bound
    rejects all eight."""
    for (C, H, W), dtype in _cpu_cases():
        f1, f2 = _features(C, H, W, dtype, False)
        l0 = R.standin_build(f1, f2, dtype, nlev=1, mutation="truncated_rounding")[0].double()
        ref = torch.einsum("npc,nqc->npq", f1.double().flatten(1, 2) / 4, f2.double().flatten(1, 2) / 4).view(N, H, W, H, W)
        eps = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
        assert torch.all((l0 - ref).abs() <= 1.01 * eps * ref.abs().clamp(min=2.0 ** -14) + 1e-4), (C, H, W, dtype)
        with pytest.raises(AssertionError, match="over the bound"):
            R.check_level0(l0.to(dtype), f1, f2, "truncated %s %s" % ((C, H, W), dtype))


@pytest.mark.parametrize("shape", [(8, 64), (11, 19), (5, 7)], ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_integer_case_is_exact_and_exercises_the_rounding(shape, dtype):
    H, W = shape
    f1, f2 = _features(128, H, W, dtype, True)
    ref, A = R.level0_ref(f1, f2)
    assert float(A.max()) * 16 < 2.0 ** 24                                   # every fp32 partial sum is exact in any order
    assert bool((ref.to(torch.bfloat16).double() != ref).any())              # level 0 holds values bf16 cannot store: the rounding is exercised
    assert float(ref.abs().max()) >= 32                                      # not trivially small
    want = R.int_want(f1, f2, dtype)
    clean = R.standin_build(f1, f2, dtype)
    for l in range(4):
        R.assert_bits(clean[l], want[l], "clean stand-in, integer features, level %d" % l)
    for m in R.MUTATIONS:
        if m in ("truncated_rounding", "pooled_from_unrounded") and dtype == torch.float16:
            continue                      # (|16 level 0| < 2^11 here: fp16 stores this level 0 exactly, so there is no rounding to get wrong)
        got = R.standin_build(f1, f2, dtype, mutation=m)
        with pytest.raises(AssertionError, match="elements differ"):
            for l in range(4):
                R.assert_bits(got[l], want[l], m)


def test_layout_helpers_invert_each_other():
    H, W = 11, 19
    for l in range(4):
        Hl, Wl = H >> l, W >> l
        m = R.inside_mask(H, W, l)
        assert int(m.sum()) == Hl * Wl
        t = torch.full((1, 1, 1) + tuple(m.shape), -1.0)
        plane = torch.arange(Hl * Wl, dtype=torch.float32).view(Hl, Wl)
        for y in range(Hl):
            for x in range(Wl):
                t[0, 0, 0, y // 8, x // 8, y % 8, x % 8] = plane[y, x]
        assert torch.equal(R.untile(t, Hl, Wl)[0, 0, 0], plane) and bool((t[0, 0, 0][~m] == -1).all()) and bool((t[0, 0, 0][m] >= 0).all())


# ------------------------------------------------------------------------------------------------ GPU plumbing
def _build(dev, f1, f2, nlev=4, guard_inputs=False):
    from pvo_amd import droid_backends as db
    a, b = f1.to(dev), f2.to(dev)
    if guard_inputs:
        g = (2 * f1.shape[2] + 2) * f1.shape[3]
        a, b = B.guarded_copy(a, g), B.guarded_copy(b, g)
    out = db.corr_build(a, b, nlev, channels_last=True)
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


def _held(levels, what):
    for l, x in enumerate(levels):
        assert not bool(torch.isnan(x.float()).any()), "%s: NaN in level %d" % (what, l)


def _check_dense(levels, f1, f2, what):
    """the three checks on random features: shapes, level-0 bound, pooled equality"""
    n, H, W, _ = f1.shape
    R.check_shapes(levels, n, H, W)
    _held(levels, what)
    worst = R.check_level0(levels[0], f1, f2, what)
    R.check_pooled(levels, what)
    return worst


def _check_int(levels, f1, f2, what):
    want = R.int_want(f1, f2, levels[0].dtype, len(levels))
    for l, x in enumerate(levels):
        R.assert_bits(x, want[l], "%s: integer features, level %d" % (what, l))


def _sentinel_levels(dev, shapes, dtype, offset=0):
    """level tensors filled with the sentinel inside NaN-filled allocations; offset: elements the views start past a 16-byte boundary"""
    bufs, views = [], []
    for s in shapes:
        n = 1
        for v in s:
            n *= v
        g = B.Guarded(n + 64, dtype, dev, 4096)
        g.inner[offset:offset + n].view(torch.int16).fill_(R.SENTINEL)
        bufs.append((g, offset, n))
        views.append(g.inner[offset:offset + n].view(*s))
    return bufs, views


def _around_untouched(bufs):
    for g, off, n in bufs:
        if not g.guards_untouched() or not bool(torch.isnan(g.inner[:off]).all()) or not bool(torch.isnan(g.inner[off + n:]).all()):
            return False
    return True


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int16) == R.SENTINEL).all())


def _i32(dev, values):
    return torch.tensor(values, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------ matrix-core path, row-major
ROW_MAJOR = [(128, s) for s in [(8, 64), (16, 64), (9, 64), (8, 40), (16, 33), (11, 19), (5, 7), (3, 5), (1, 1)]] + \
            [(c, s) for c in (16, 32, 64) for s in [(8, 64), (11, 19), (5, 7)]]


@gpu
@pytest.mark.parametrize("C,shape", ROW_MAJOR, ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_row_major_build_every_epilogue(cuda, dtype, C, shape):
    """(8, 64), (16, 64): the aligned epilogue, one and two patch rows, level 3 one and two rows high; (9, 64), (8, 40), (16, 33):
    ragged because of H, because of W, one column into a second patch; (11, 19): HW = 209 - a wave with 17 source pixels whose second
    half holds one row, and an empty wave; (5, 7): smaller than a patch, level 3 empty with a NULL pointer, a wave with 3 rows;
    (3, 5): HW = 15 < 16, second half empty; (1, 1): levels 1..3 empty."""
    H, W = shape
    what = "row-major C=%d %dx%d %s" % (C, H, W, _id(dtype))
    f1, f2 = _features(C, H, W, dtype, False)
    got = _build(cuda, f1, f2)
    _check_dense(got, f1, f2, what)
    guarded = _build(cuda, f1, f2, guard_inputs=True)
    _held(guarded, what + ", guarded inputs")
    for l in range(4):
        R.assert_bits(guarded[l], got[l], "%s: level %d with guarded inputs" % (what, l))
    i1, i2 = _features(C, H, W, dtype, True)
    _check_int(_build(cuda, i1, i2), i1, i2, what)


@gpu
@pytest.mark.parametrize("shape", [(8, 64), (11, 19)], ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_row_major_fewer_levels_are_the_first_levels_of_four(cuda, dtype, shape):
    """num_levels < 4 sends an aligned shape through the ragged writer"""
    H, W = shape
    f1, f2 = _features(128, H, W, dtype, False)
    full = _build(cuda, f1, f2)
    _check_dense(full, f1, f2, "four levels %dx%d %s" % (H, W, _id(dtype)))
    for nlev in (1, 2, 3):
        got = _build(cuda, f1, f2, nlev)
        assert len(got) == nlev
        for l in range(nlev):
            R.assert_bits(got[l], full[l], "num_levels=%d, level %d" % (nlev, l))
        guarded = _build(cuda, f1, f2, nlev, guard_inputs=True)
        for l in range(nlev):
            R.assert_bits(guarded[l], full[l], "num_levels=%d, guarded inputs, level %d" % (nlev, l))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_row_major_misaligned_levels_take_the_ragged_writer(cuda, dtype):
    """level tensors that start 2 bytes past a 16-byte boundary inside larger NaN-filled allocations: same bits as the aligned call,
    nothing around the views touched"""
    from pvo_amd import droid_backends as db
    H, W, C = 8, 64, 128
    f1, f2 = _features(C, H, W, dtype, False)
    full = _build(cuda, f1, f2)
    _check_dense(full, f1, f2, "aligned call 8x64 %s" % _id(dtype))
    for guard_inputs in (False, True):
        bufs, views = _sentinel_levels(cuda, [(N, H, W, H >> l, W >> l) for l in range(4)], dtype, offset=1)
        assert all(v.data_ptr() % 16 == 2 and v.is_contiguous() for v in views)
        a, b = f1.to(cuda), f2.to(cuda)
        if guard_inputs:
            a, b = B.guarded_copy(a, (2 * W + 2) * C), B.guarded_copy(b, (2 * W + 2) * C)
        db.corr_build(a, b, 4, channels_last=True, out=views, out_slots=_i32(cuda, [0, 1]))
        torch.cuda.synchronize()
        assert _around_untouched(bufs)
        for l in range(4):
            R.assert_bits(views[l], full[l], "misaligned level %d" % l)


@gpu
@pytest.mark.parametrize("shape", [(8, 64), (6, 24)], ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_row_major_out_slots_write_their_slots_only(cuda, dtype, shape):
    """what a non-tiled CorrVolumePool calls: capacity 5, edges 0 and 1 into slots 4 and 0"""
    from pvo_amd import droid_backends as db
    H, W = shape
    C = 128
    f1, f2 = _features(C, H, W, dtype, False)
    dense = _build(cuda, f1, f2)
    _check_dense(dense, f1, f2, "dense call %dx%d %s" % (H, W, _id(dtype)))
    for guard_inputs in (False, True):
        bufs, lv = _sentinel_levels(cuda, [(5, H, W, H >> l, W >> l) for l in range(4)], dtype)
        a, b = f1.to(cuda), f2.to(cuda)
        if guard_inputs:
            a, b = B.guarded_copy(a, (2 * W + 2) * C), B.guarded_copy(b, (2 * W + 2) * C)
        db.corr_build(a, b, 4, channels_last=True, out=lv, out_slots=_i32(cuda, [4, 0]))
        torch.cuda.synchronize()
        assert _around_untouched(bufs)
        for l in range(4):
            if lv[l].numel() == 0:
                continue
            R.assert_bits(lv[l][[4, 0]], dense[l], "slots [4, 0], level %d" % l)
            assert _is_sentinel(lv[l][1:4]), "level %d: an unused slot was written" % l


# ------------------------------------------------------------------------------------------------ tiled path
TILED = [(128, s) for s in [(8, 8), (8, 64), (9, 17), (17, 9), (16, 24), (11, 19), (24, 40)]] + \
        [(c, s) for c in (16, 64) for s in [(9, 17), (8, 64)]]
CAP, SLOTS, UNUSED = 5, [4, 0], [1, 2, 3]


def _tiled_levels(dev, H, W, dtype):
    from pvo_amd import droid_backends as db
    return _sentinel_levels(dev, [(CAP, H, W) + db.tiled_level_shape(H, W, l) for l in range(4)], dtype)


def _untiled(bufs, lv, H, W, what):
    """guards and unused slots untouched; the used slots' planes, un-tiled on the host"""
    torch.cuda.synchronize()
    assert _around_untouched(bufs), what
    out = []
    for l in range(4):
        t = lv[l].cpu()
        assert _is_sentinel(t[UNUSED]), "%s: level %d, an unused slot was written" % (what, l)
        m = R.inside_mask(H, W, l)
        assert not bool((t[SLOTS][..., m].view(torch.int16) == R.SENTINEL).any()), "%s: level %d has unwritten elements" % (what, l)
        out.append(R.untile(t[SLOTS], H >> l, W >> l))
    return out


@gpu
@pytest.mark.parametrize("C,shape", TILED, ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_tiled_build_directly_against_fp64(cuda, dtype, C, shape):
    from pvo_amd import droid_backends as db
    H, W = shape
    what = "tiled C=%d %dx%d %s" % (C, H, W, _id(dtype))
    slots = _i32(cuda, SLOTS)
    f1, f2 = _features(C, H, W, dtype, False)
    bufs, lv = _tiled_levels(cuda, H, W, dtype)
    db.corr_build_tiled(f1.to(cuda), f2.to(cuda), lv, slots)
    got = _untiled(bufs, lv, H, W, what)
    _check_dense(got, f1, f2, what)
    bufs, lv = _tiled_levels(cuda, H, W, dtype)
    g = (2 * W + 2) * C
    db.corr_build_tiled(B.guarded_copy(f1.to(cuda), g), B.guarded_copy(f2.to(cuda), g), lv, slots)
    guarded = _untiled(bufs, lv, H, W, what + ", guarded inputs")
    _held(guarded, what + ", guarded inputs")
    for l in range(4):
        R.assert_bits(guarded[l], got[l], "%s: level %d with guarded inputs" % (what, l))
    i1, i2 = _features(C, H, W, dtype, True)
    bufs, lv = _tiled_levels(cuda, H, W, dtype)
    db.corr_build_tiled(i1.to(cuda), i2.to(cuda), lv, slots)
    _check_int(_untiled(bufs, lv, H, W, what + ", integer"), i1, i2, what)


ROWS1, ROWS2 = [3, 1], [2, 2]


def _frames(dev, f, rows, C, W):
    """[4, H, W, C] between NaN guards: frame rows[k] holds f[k], every frame no row names is NaN"""
    fr = torch.full((4,) + tuple(f.shape[1:]), float("nan"), dtype=f.dtype)
    for k, r in enumerate(rows):
        fr[r] = f[k]
    return B.guarded_copy(fr.to(dev), (2 * W + 2) * C)


@gpu
@pytest.mark.parametrize("C,shape", TILED, ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_tiled_rows_build_directly_against_fp64(cuda, dtype, C, shape):
    """edge k reads frame ROWS1[k] of the first buffer and frame ROWS2[k] of the second; the reference is that of the gathered frames.
    Frames no row names are NaN, and no NaN may reach an output."""
    from pvo_amd import droid_backends as db
    H, W = shape
    what = "tiled rows C=%d %dx%d %s" % (C, H, W, _id(dtype))
    for integer in (False, True):
        f1, f2 = _features(C, H, W, dtype, integer)
        f2 = f2[[0, 0]]                                                   # both edges read frame 2 of the second buffer
        bufs, lv = _tiled_levels(cuda, H, W, dtype)
        db.corr_build_tiled_rows(_frames(cuda, f1, ROWS1, C, W), _frames(cuda, f2, ROWS2, C, W), _i32(cuda, ROWS1), _i32(cuda, ROWS2),
                                 lv, _i32(cuda, SLOTS))
        got = _untiled(bufs, lv, H, W, what)
        if integer:
            _check_int(got, f1, f2, what)
        else:
            _check_dense(got, f1, f2, what)


# ------------------------------------------------------------------------------------------------ generic path
GENERIC_SHAPES = [(9, 13), (5, 7), (8, 9), (1, 1)]
ALL_DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]


def _generic_build(dev, f1, f2, nlev, channels_last, guard_inputs=False):
    from pvo_amd import droid_backends as db
    a, b = f1.to(dev), f2.to(dev)
    if not channels_last:
        a, b = a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous()
    if guard_inputs:
        g = (2 * f1.shape[2] + 2) * f1.shape[3]
        a, b = B.guarded_copy(a, g), B.guarded_copy(b, g)
    out = db.corr_build(a, b, nlev, channels_last=channels_last)
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


@gpu
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=_id)
def test_generic_build_bounds_and_exact_pooling(cuda, dtype, channels_last):
    """odd channel counts force the generic kernels for the 16-bit types too.  fp32 / fp64: a chain of C fused multiply-adds and no
    storage rounding; pooled levels equal pool_exact in every type."""
    worst = 0.0
    for C in (1, 17, 24):
        for H, W in GENERIC_SHAPES:
            what = "generic %s %s C=%d %dx%d" % (_id(dtype), "nhwc" if channels_last else "nchw", C, H, W)
            f1, f2 = _features(C, H, W, dtype, False)
            full = _generic_build(cuda, f1, f2, 4, channels_last)
            worst = max(worst, _check_dense(full, f1, f2, what))
            guarded = _generic_build(cuda, f1, f2, 4, channels_last, guard_inputs=True)
            for l in range(4):
                R.assert_bits(guarded[l], full[l], "%s: level %d with guarded inputs" % (what, l))
            for nlev in (1, 2, 3):
                got = _generic_build(cuda, f1, f2, nlev, channels_last)
                assert len(got) == nlev
                for l in range(nlev):
                    R.assert_bits(got[l], full[l], "%s: num_levels=%d, level %d" % (what, nlev, l))
    print("generic %s %s: largest err / bound = %.3g" % (_id(dtype), "nhwc" if channels_last else "nchw", worst))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_misaligned_feature_view_falls_through_to_the_generic_kernel(cuda, dtype):
    """a channels-last 16-bit feature view 2 bytes past a 16-byte boundary cannot feed the matrix-core kernel's 16-byte loads"""
    C, H, W = 64, 9, 13
    f1, f2 = _features(C, H, W, dtype, False)
    n = f1.numel()
    views = []
    for f in (f1, f2):
        g = B.Guarded(n + 64, dtype, cuda, (2 * W + 2) * C)
        v = g.inner[1:1 + n].view(N, H, W, C)
        v.copy_(f)
        assert v.data_ptr() % 16 == 2 and v.is_contiguous()
        views.append(v)
    from pvo_amd import droid_backends as db
    got = db.corr_build(views[0], views[1], 4, channels_last=True)
    torch.cuda.synchronize()
    _check_dense([x.cpu() for x in got], f1, f2, "misaligned features C=64 9x13 %s" % _id(dtype))


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=_id)
def test_generic_path_refuses_out_slots_and_writes_nothing(cuda, dtype):
    from pvo_amd import droid_backends as db
    C, H, W = 24, 5, 7
    f1, f2 = _features(C, H, W, dtype, False)
    lv = [torch.full((5, H, W, H >> l, W >> l), 7.5, dtype=dtype, device=cuda) for l in range(4)]
    with pytest.raises(db.PvoHipError):
        db.corr_build(f1.to(cuda), f2.to(cuda), 4, channels_last=True, out=lv, out_slots=_i32(cuda, [4, 0]))
    torch.cuda.synchronize()
    assert all(bool((x == 7.5).all()) for x in lv)


# ------------------------------------------------------------------------------------------------ refusals of the C entry points
OK, EINVAL, EUNSUPPORTED = 0, 1, 4


@gpu
def test_entry_points_refuse_bad_arguments_and_write_nothing(cuda):
    from pvo_amd import _lib
    lib = _lib.load()
    C, H, W, F16 = 16, 8, 8, _lib.PVO_F16
    big = torch.full((2 * 8 * 8 * 256 + 8,), 0.5, dtype=torch.float16, device=cuda)          # features: room for every C asked below
    rows = _i32(cuda, [0, 0])
    slots = _i32(cuda, [0, 0])
    bufs_r, lv_r = _sentinel_levels(cuda, [(1, H, W, H >> l, W >> l) for l in range(4)], torch.float16)
    from pvo_amd import droid_backends as db
    bufs_t, lv_t = _sentinel_levels(cuda, [(1, H, W) + db.tiled_level_shape(H, W, l) for l in range(4)], torch.float16)
    f = big.data_ptr()
    assert f % 16 == 0
    pr = [x.data_ptr() for x in lv_r]
    pt = [x.data_ptr() for x in lv_t]
    arr = lambda p: (ctypes.c_void_p * 4)(*p)
    null1 = lambda p: arr([p[0], None, p[2], p[3]])

    def build(f1=f, f2=f, lv=arr(pr), n=1, c=C, h=H, w=W, nlev=4, dt=F16, cl=1):
        return lib.pvo_corr_build(f1, f2, lv, n, c, h, w, nlev, dt, cl, None, None)

    def tiled(f1=f, f2=f, lv=arr(pt), n=1, c=C, h=H, w=W):
        return lib.pvo_corr_build_tiled(f1, f2, lv, n, c, h, w, F16, slots.data_ptr(), None)

    def trows(f1=f, f2=f, r1=rows.data_ptr(), r2=rows.data_ptr(), lv=arr(pt), n=1, c=C, h=H, w=W):
        return lib.pvo_corr_build_tiled_rows(f1, f2, r1, r2, lv, n, c, h, w, F16, slots.data_ptr(), None)

    for cl, dt in ((1, F16), (0, _lib.PVO_F32)):                         # in front of the matrix-core path and of the generic one
        for kw in (dict(n=-1), dict(c=0), dict(c=-3), dict(nlev=0), dict(nlev=5), dict(lv=None), dict(lv=null1(pr)), dict(f1=None),
                   dict(f2=None), dict(n=65536)):
            assert build(cl=cl, dt=dt, **kw) == EINVAL, ("pvo_corr_build", kw)
        for kw in (dict(n=0), dict(h=0), dict(w=0)):
            assert build(cl=cl, dt=dt, **kw) == OK, ("pvo_corr_build", kw)
    for name, fn in (("pvo_corr_build_tiled", tiled), ("pvo_corr_build_tiled_rows", trows)):
        for kw in (dict(n=-1), dict(c=0), dict(lv=None), dict(lv=null1(pt)), dict(f1=None), dict(n=65536)):
            assert fn(**kw) == EINVAL, (name, kw)
        for kw in (dict(n=0), dict(h=0), dict(w=0)):
            assert fn(**kw) == OK, (name, kw)
        for kw in (dict(c=24), dict(c=256), dict(h=7), dict(lv=arr([pt[0], pt[1] + 2, pt[2], pt[3]])), dict(f1=f + 2), dict(f2=f + 2)):
            assert fn(**kw) == EUNSUPPORTED, (name, kw)
    assert trows(r1=None) == EINVAL and trows(r2=None) == EINVAL
    torch.cuda.synchronize()
    assert _around_untouched(bufs_r) and _around_untouched(bufs_t)
    assert all(_is_sentinel(x) for x in lv_r + lv_t) and bool((big == 0.5).all())


# ------------------------------------------------------------------------------------------------ the pool
def _coords(g, n, H, W, dev):
    return (torch.rand(1, n, H, W, 2, generator=g) * torch.tensor([W + 4.0, H + 4.0]) - 2.0).to(dev)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_row_major_pool_matches_corrblock_through_edge_changes(cuda, dtype):
    """a map under 8 pixels high: CorrVolumePool keeps row-major planes and builds through out_slots"""
    from pvo_amd.modules.corr import CorrBlock, CorrVolumePool
    g = torch.Generator().manual_seed(5)
    H, W, C = 6, 24, 64
    f = torch.randn(6, H, W, C, generator=g).to(dtype).to(cuda)
    ii, jj = [0, 1, 2, 3, 4], [1, 2, 3, 4, 5]
    pool = CorrVolumePool(8, H, W, cuda, dtype)
    assert not pool.tiled
    pool.add(f[ii], f[jj])
    blk = CorrBlock(f[ii][None], f[jj][None], channels_last=True)
    keep = [True, False, True, True, False]
    pool.keep(keep)
    blk = blk[torch.tensor(keep, device=cuda)]
    pool.add(f[[5, 0]], f[[0, 3]])
    blk = blk.cat(CorrBlock(f[[5, 0]][None], f[[0, 3]][None], channels_last=True))
    assert len(pool) == 5 and sorted(pool.slots + pool.free) == list(range(8))
    coords = _coords(g, 5, H, W, cuda)
    for cl in (False, True):
        a, b = pool(coords, channels_last=cl), blk(coords, channels_last=cl)
        assert a.shape == b.shape == (1, 5, 196, H, W)
        R.assert_bits(a, b, "row-major pool against CorrBlock")
    R.check_level0(pool.levels[0][pool.slots[3:]], f[[5, 0]].cpu(), f[[0, 3]].cpu(), "row-major pool, re-added edges %s" % _id(dtype))


@gpu
@pytest.mark.parametrize("shape,tiled", [((16, 24), True), ((6, 24), False)], ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_pool_growth_keeps_live_slots_and_builds_into_new_ones(cuda, dtype, shape, tiled):
    from pvo_amd.modules.corr import CorrVolumePool
    H, W = shape
    C = 64
    g = torch.Generator().manual_seed(H)
    f = torch.randn(6, H, W, C, generator=g).to(dtype).to(cuda)
    small, big = CorrVolumePool(3, H, W, cuda, dtype), CorrVolumePool(8, H, W, cuda, dtype)
    assert small.tiled == tiled and big.tiled == tiled
    for pool in (small, big):
        pool.add(f[[0, 1, 2]], f[[1, 2, 3]])
    before = [lv[small.slots].clone() for lv in small.levels]
    for pool in (small, big):
        pool.add(f[[3]], f[[4]])
        pool.add(f[[4]], f[[5]])
    assert small.capacity >= 5 and len(small) == 5 and len(set(small.slots)) == 5 and big.capacity == 8
    assert sorted(small.slots + small.free) == list(range(small.capacity))
    for l in range(4):
        R.assert_bits(small.levels[l][small.slots[:3]], before[l], "level %d of the live slots across the growth" % l)
    new = [lv[small.slots[3:]].cpu() for lv in small.levels]
    if tiled:
        new = [R.untile(new[l], H >> l, W >> l) for l in range(4)]
    _check_dense(new, f[[3, 4]].cpu(), f[[4, 5]].cpu(), "grown %s pool %dx%d %s" % ("tiled" if tiled else "row-major", H, W, _id(dtype)))
    coords = _coords(g, 5, H, W, cuda)
    for cl in (False, True):
        R.assert_bits(small(coords, channels_last=cl), big(coords, channels_last=cl), "lookup of the grown pool")


@gpu
def test_fp32_pool_can_be_filled_and_matches_corrblock(cuda):
    """pvo_corr_build serves fp32 on its generic path, which has no slot output: the pool builds densely and copies into its slots"""
    from pvo_amd.modules.corr import CorrBlock, CorrVolumePool
    H, W, C = 16, 24, 32
    g = torch.Generator().manual_seed(32)
    f = torch.randn(3, H, W, C, generator=g).to(cuda)
    pool = CorrVolumePool(3, H, W, cuda, torch.float32)
    assert not pool.tiled
    for lv in pool.levels:
        lv.fill_(float("nan"))
    pool.add(f[[0, 1]], f[[1, 2]])
    blk = CorrBlock(f[[0, 1]][None], f[[1, 2]][None], channels_last=True)
    assert len(pool) == 2 and sorted(pool.slots + pool.free) == [0, 1, 2]
    for l in range(4):
        R.assert_bits(pool.levels[l][pool.slots], blk.corr_pyramid[l], "fp32 pool, level %d" % l)
        assert bool(torch.isnan(pool.levels[l][pool.free]).all()), "fp32 pool, level %d: the free slot was written" % l
    coords = _coords(g, 2, H, W, cuda)
    for cl in (False, True):
        R.assert_bits(pool(coords, channels_last=cl), blk(coords, channels_last=cl), "fp32 pool against CorrBlock")
    _check_dense([lv[pool.slots].cpu() for lv in pool.levels], f[[0, 1]].cpu(), f[[1, 2]].cpu(), "fp32 pool 16x24")
