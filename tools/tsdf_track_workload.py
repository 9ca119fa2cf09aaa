"""The tracker's kernels one by one: 64 slots, 10 iterations, the dense 256^3 volume of tools/tsdf_track_bench.py, eight calls at 48 x 64
and eight at 384 x 512 - the workload of a kernel trace:

    rocprofv3 --kernel-trace -f csv -d DIR -o track -- python tools/tsdf_track_workload.py

and the medians of track_pixels_kernel / track_solve_kernel per image size from DIR's kernel trace -> profiles/r25_tsdf_track_kernels.txt.
Needs the GPU: there is no fallback."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tsdf_bench import make_video  # noqa: E402
from pvo_amd import droid_backends as db  # noqa: E402

dev = torch.device("cuda:0")
nf, dim = 64, 256
voxel = 2.56 / dim
origin = (-1.28, -1.28, 0.5)
poses, disps, intr, _ = make_video(nf, 48, 64, dev)
ix = torch.arange(nf, device=dev)
tsdf, wsum = torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev)
db.tsdf_integrate(tsdf, wsum, None, poses, disps, intr, ix, origin, voxel, 3 * voxel)
for ht, wd in ((48, 64), (384, 512)):
    p, d, k, _ = make_video(nf, ht, wd, dev)
    for _ in range(8):
        db.tsdf_track(tsdf, wsum, origin, voxel, p, d, k, ix, iters=10)
    torch.cuda.synchronize()
print("done")
