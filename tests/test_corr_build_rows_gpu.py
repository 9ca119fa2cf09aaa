"""pvo_corr_build_tiled_rows: the tiled volume build reading frames rows1[n] / rows2[n] of per-frame feature buffers writes, in
every level, the bits pvo_corr_build_tiled writes given the gathered feature maps."""
import pytest
import torch

C, N, F, CAP = 128, 3, 4, 5
ROWS1, ROWS2, SLOTS = [3, 1, 1], [2, 2, 0], [4, 0, 2]         # a repeated and a descending index; slots out of order, two left free


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(8, 40), (16, 64)])
def test_indexed_volume_build_equals_the_gathered_call(cuda, dt, H, W):
    from pvo_amd import droid_backends as db
    g = torch.Generator().manual_seed(H + W)
    f1 = torch.randn(F, H, W, C, generator=g).to(dt).to(cuda)
    f2 = torch.randn(F, H, W, C, generator=g).to(dt).to(cuda)
    i32 = lambda l: torch.tensor(l, dtype=torch.int32, device=cuda)
    rows1, rows2, slots = i32(ROWS1), i32(ROWS2), i32(SLOTS)
    levels = lambda: [torch.zeros((CAP, H, W) + db.tiled_level_shape(H, W, l), dtype=dt, device=cuda) for l in range(4)]
    want = db.corr_build_tiled(f1[rows1.long()].contiguous(), f2[rows2.long()].contiguous(), levels(), slots)
    got = db.corr_build_tiled_rows(f1, f2, rows1, rows2, levels(), slots)
    torch.cuda.synchronize()
    for l in range(4):
        assert torch.equal(got[l], want[l]), "level %d" % l
        assert want[l][SLOTS].float().abs().max() > 0 and not want[l][[1, 3]].any()       # written where told, nowhere else
    # both sides from ONE buffer (what the factor graph passes: video.fmaps twice)
    want = db.corr_build_tiled(f1[rows1.long()].contiguous(), f1[rows2.long()].contiguous(), levels(), slots)
    got = db.corr_build_tiled_rows(f1, f1, rows1, rows2, levels(), slots)
    for l in range(4):
        assert torch.equal(got[l], want[l]), "level %d, one buffer" % l


@pytest.mark.gpu
def test_indexed_volume_build_checks_its_tables(cuda):
    from pvo_amd import droid_backends as db
    H, W = 8, 40
    f = torch.zeros(F, H, W, C, dtype=torch.float16, device=cuda)
    lv = [torch.zeros((CAP, H, W) + db.tiled_level_shape(H, W, l), dtype=torch.float16, device=cuda) for l in range(4)]
    i32 = lambda l: torch.tensor(l, dtype=torch.int32, device=cuda)
    with pytest.raises(db.PvoHipError):
        db.corr_build_tiled_rows(f, f, i32(ROWS1), i32(ROWS2).long(), lv, i32(SLOTS))
    with pytest.raises(db.PvoHipError):
        db.corr_build_tiled_rows(f, f, i32(ROWS1), i32(ROWS2[:2]), lv, i32(SLOTS))
