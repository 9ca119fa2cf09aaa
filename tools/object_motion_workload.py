"""pvo_object_motion's kernels one by one: tools/object_motion_bench.py's window with 16 jobs per edge (768 jobs), iters = 8, 20 calls.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o om -- python tools/object_motion_workload.py

then `python tools/object_motion_bench.py --kernel-stats DIR/.../om_kernel_stats.csv` copies the three kernels' rows into
profiles/r29_object_motion.txt.  Needs the GPU."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from object_motion_bench import make_operands  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("object_motion_workload needs the GPU")
    from pvo_amd import droid_backends as db
    dev = torch.device("cuda:0")
    ops = make_operands(dev)
    E = ops["ii"].shape[0]
    job_edge = torch.arange(E, device=dev).repeat_interleave(16).contiguous()
    job_label = (1 + torch.arange(16, device=dev, dtype=torch.int32)).repeat(E).contiguous()
    for _ in range(20):
        db.object_motion(ops["poses"], ops["disps"], ops["intrinsics"], ops["labels"], ops["ii"], ops["jj"], ops["target"], job_edge, job_label, iters=8)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
