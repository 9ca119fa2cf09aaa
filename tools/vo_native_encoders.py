"""tools/test_vo.py with `--native_encoders`: the per-frame encoders' 3 x 3 / 7 x 7 convolutions on the library's own deterministic
kernel (pvo_conv_planes) instead of the vendor library.

    python tools/vo_native_encoders.py --datapath <sequence> [every other argument of tools/test_vo.py] [--native_encoders]

The driver itself stays the reference's (tools/test_vo.py is not edited): this entry point parses the one extra switch, hands the
rest to test_vo.parse_args and runs test_vo.main with `args.native_encoders` set - the field `Droid` reads.  The switch defaults to ON
here (that is what this entry point is for); `--no_native_encoders` runs the vendor path through the same code for an A/B."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vo  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--native_encoders", dest="native_encoders", action="store_true", default=True,
                   help="the encoders' convolutions on pvo_conv_planes (default here)")
    p.add_argument("--no_native_encoders", dest="native_encoders", action="store_false", help="keep the vendor library's convolutions")
    own, rest = p.parse_known_args(argv)
    args = test_vo.parse_args(rest)
    args.native_encoders = own.native_encoders
    return args


def main(argv=None):
    args = parse_args(argv)
    plain = test_vo.parse_args
    test_vo.parse_args = lambda _argv=None: args          # (test_vo.main parses for itself: hand it the namespace with the switch)
    try:
        test_vo.main(argv)
    finally:
        test_vo.parse_args = plain


if __name__ == "__main__":
    main()
