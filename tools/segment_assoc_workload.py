"""pvo_segment_associate's kernels one by one: tools/segment_assoc_bench.py's window, 20 calls at one S and form.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o sa -- python tools/segment_assoc_workload.py S [FORM]

S: 16, 64, 160 or 128 (the bench's grids); FORM: 0 (as the library picks) or 1 (the table in LDS, S <= 128).  The three kernels' rows of
DIR/.../sa_kernel_stats.csv are what profiles/r30_segment_assoc_kernels.txt records.  Needs the GPU."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from segment_assoc_bench import make_labels, make_operands  # noqa: E402


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise SystemExit("segment_assoc_workload needs the GPU")
    from pvo_amd import droid_backends as db
    S, form = int(argv[0]), int(argv[1]) if len(argv) > 1 else 0
    dev = torch.device("cuda:0")
    ops = make_operands(dev)
    labels = make_labels(S, dev)
    for _ in range(20):
        db.segment_associate(labels, ops["ii"], ops["jj"], ops["target"], S, form=form)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
