"""The host side of pvo_conv_planes (no GPU needed): which shapes it takes, the size of a packed filter, the ABI version."""
import itertools


def _rule(ksize, stride, cin, cout):
    """include/pvo_hip.h: 3 x 3 with stride 1 or 2 and Cin, Cout positive multiples of 32; 7 x 7 stride 2 with Cin = 3, Cout a multiple of 32"""
    if cout <= 0 or cout % 32:
        return False
    if ksize == 3:
        return stride in (1, 2) and cin > 0 and cin % 32 == 0
    if ksize == 7:
        return stride == 2 and cin == 3
    return False


def test_supported_shapes_follow_the_rule_of_the_header():
    from pvo_amd import droid_backends as db
    n = 0
    for k, s, ci, co in itertools.product((1, 3, 5, 7, 9), (0, 1, 2, 3, 4), (0, 1, 3, 8, 16, 32, 48, 64, 96, 128, 256), (0, 8, 32, 40, 64, 128, 256, 264)):
        assert db.conv_planes_supported(k, s, ci, co) == _rule(k, s, ci, co), (k, s, ci, co)
        n += _rule(k, s, ci, co)
    assert n == 2 * 5 * 4 + 4                                     # (the grid does reach the supported shapes: 3 x 3 and the stem)
    # every convolution of the two encoders that is not 1 x 1
    for k, s, ci, co in ((7, 2, 3, 32), (3, 1, 32, 32), (3, 2, 32, 64), (3, 1, 64, 64), (3, 2, 64, 128), (3, 1, 128, 128)):
        assert db.conv_planes_supported(k, s, ci, co)


def test_packed_filter_size_and_abi_version():
    from pvo_amd import _lib
    lib = _lib.load()
    assert lib.pvo_version() == 106 == _lib.PVO_ABI_VERSION
    for k, ci, co in ((3, 32, 32), (3, 32, 64), (3, 64, 64), (3, 64, 128), (3, 128, 128), (3, 256, 96), (7, 3, 32), (7, 3, 64)):
        nbytes = lib.pvo_conv_planes_filter_bytes(k, ci, co)
        padded_k = -(-(ci * k * k) // 32) * 32                      # K padded to the MFMA's 32
        assert nbytes >= padded_k * co * 2 and nbytes % 16 == 0, (k, ci, co, nbytes)
    for k, ci, co in ((5, 32, 32), (3, 48, 32), (3, 32, 40), (7, 4, 32), (7, 3, 48)):
        assert lib.pvo_conv_planes_filter_bytes(k, ci, co) == 0


def test_command_line_switch_reaches_droid_args():
    """tools/vo_native_encoders.py: tools/test_vo.py's arguments plus the switch `Droid` reads (args.native_encoders)"""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import vo_native_encoders as v
    finally:
        sys.path.remove(tools)
    a = v.parse_args(["--native_encoders", "--datapath", "x", "--buffer", "64", "--pipelined"])
    assert a.native_encoders is True and a.datapath == "x" and a.buffer == 64 and a.pipelined is True
    assert v.parse_args(["--datapath", "x"]).native_encoders is True
    assert v.parse_args(["--no_native_encoders", "--datapath", "x"]).native_encoders is False
    from pvo_amd.droid import default_args
    assert getattr(default_args(), "native_encoders", False) is False          # the library's default stays off
