"""The wide 3x3 convolution (conv3x3_big_kernel: 16x16 pixel tile x 128 outputs per workgroup, v_mfma_f32_16x16x32) at
the widths that pick each main-loop instantiation and their neighbours, through all four entry points that launch it
(pvo_conv3x3, pvo_gru_conv_gates / _candidate, pvo_conv3x3_heads), against torch fp32 convolutions on the same 16-bit
inputs at the tolerances of tests/test_update_operator.py."""
import pytest
import torch
import torch.nn.functional as F

CL = torch.channels_last
# S-B (36 x 48 x 64 in the benchmark; fewer edges here), very narrow maps, one full tile column and a half, the reference
# driver's 101 (a right-most tile with 5 valid columns: the half main loop), and 16 k - 1 / 16 k + 1 (the last tile
# with 15 valid columns, the full loop; with 1 valid column, the half loop)
SHAPES = [(3, 48, 64), (2, 9, 5), (1, 13, 7), (2, 20, 24), (1, 30, 101), (1, 17, 31), (1, 18, 33), (2, 7, 47), (1, 5, 49)]


def _tol(dt):
    return 4e-3 if dt == torch.float16 else 3e-2


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,H,W", SHAPES)
def test_wide_conv_plain_and_channel_slice(cuda, dt, E, H, W):
    from pvo_amd import droid_backends as db
    g = torch.Generator().manual_seed(E * 7 + H * 31 + W)
    Cin, Cout = 96, 256
    x = torch.randn(E, Cin, H, W, generator=g).to(dt).to(cuda).contiguous(memory_format=CL)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (0.5 / (9 * Cin) ** 0.5)).to(dt).to(cuda)
    b = torch.randn(Cout, generator=g).to(cuda)
    wt = db.conv3x3_weights(w, dt)
    tol = _tol(dt)
    y = db.conv3x3(x, wt, b, relu=True)
    ref = torch.relu(F.conv2d(x.float(), w.float(), b, padding=1))
    assert torch.allclose(y.float(), ref, atol=tol, rtol=tol) and (y.float() - ref).abs().mean().item() < tol / 8
    wide = torch.full((E, H, W, Cout + 128), 7.0, dtype=dt, device=cuda).permute(0, 3, 1, 2)
    y3 = db.conv3x3(x, wt, b, relu=True, out=wide, out_offset=64)
    assert torch.equal(y3, y) and (wide[:, :64] == 7).all() and (wide[:, 64 + Cout:] == 7).all()
    assert torch.equal(db.conv3x3(x, wt, b, relu=True), y)                 # bitwise the same on a second launch


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,H,W", SHAPES)
def test_wide_conv_gru_epilogues_segmented_and_slots(cuda, dt, E, H, W):
    from pvo_amd import droid_backends as db
    g_ = torch.Generator().manual_seed(E + 3 * H + 5 * W)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g_) * sc).to(dt).to(cuda)
    net = torch.tanh(r(E, 128, H, W)).contiguous(memory_format=CL)
    cf = torch.relu(r(E, 192, H, W)).contiguous(memory_format=CL)
    P_zr, P_q = r(E, 256, H, W, sc=0.3).contiguous(memory_format=CL), r(E, 128, H, W, sc=0.3).contiguous(memory_format=CL)
    gg = (torch.randn(E, 384, generator=g_) * 0.3).to(cuda)
    wzr, wq = r(256, 320, 3, 3, sc=0.02), r(128, 320, 3, 3, sc=0.02)
    tzr, tq = db.conv3x3_weights(wzr, dt), db.conv3x3_weights(wq, dt)
    Z, RN = db.gru_conv_gates(net, cf, tzr, gg, P_zr)
    out = db.gru_conv_candidate(RN, cf, tq, gg, P_q, Z, net)
    pre = F.conv2d(torch.cat([net, cf], 1).float(), wzr.float(), None, padding=1) + gg[:, :256, None, None] + P_zr.float()
    tol = _tol(dt)
    assert torch.allclose(Z.float(), torch.sigmoid(pre[:, :128]), atol=tol)
    assert torch.allclose(RN.float(), torch.sigmoid(pre[:, 128:]) * net.float(), atol=tol)
    q_ref = F.conv2d(torch.cat([RN.float(), cf.float()], 1), wq.float(), None, padding=1) + gg[:, 256:, None, None] + P_q.float()
    assert torch.allclose(out.float(), (1 - Z.float()) * net.float() + Z.float() * torch.tanh(q_ref), atol=2 * tol)
    # static terms read from a slot pool through p_slots, and a second launch: bitwise the same
    cap = E + 2
    perm = torch.randperm(cap, generator=g_)[:E].to(cuda)
    Pz_pool = torch.randn(cap, 256, H, W, device=cuda).to(dt).contiguous(memory_format=CL)
    Pq_pool = torch.randn(cap, 128, H, W, device=cuda).to(dt).contiguous(memory_format=CL)
    Pz_pool[perm] = P_zr
    Pq_pool[perm] = P_q
    slots = perm.int().contiguous()
    Z2, RN2 = db.gru_conv_gates(net, cf, tzr, gg, Pz_pool, p_slots=slots)
    out2 = db.gru_conv_candidate(RN2, cf, tq, gg, Pq_pool, Z2, net, p_slots=slots)
    assert torch.equal(Z2, Z) and torch.equal(RN2, RN) and torch.equal(out2, out)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,H,W", [(2, 48, 64), (1, 9, 5), (1, 30, 101), (1, 17, 31), (1, 6, 33)])
def test_wide_conv_heads_match_torch(cuda, dt, E, H, W):
    from pvo_amd import droid_backends as db
    g = torch.Generator().manual_seed(11 * H + W)
    x = torch.tanh(torch.randn(E, 128, H, W, generator=g)).to(cuda).to(dt).contiguous(memory_format=CL)
    w1 = (torch.randn(512, 128, 3, 3, generator=g) * 0.03).to(cuda)
    b1 = torch.randn(512, generator=g).to(cuda) * 0.1
    w = [torch.randn(2, 128, 3, 3, generator=g).to(cuda) * 0.05 for _ in range(4)]
    b2 = torch.randn(8, generator=g).to(cuda)
    w2 = torch.stack([t.permute(0, 2, 3, 1).reshape(2, 9, 128) for t in w])
    t1, f2 = db.conv3x3_weights(w1.to(dt), dt), db.heads2_fragments(w2, dt)
    y = db.heads_fused(x, t1, b1, f2, b2)
    hidden = torch.relu(F.conv2d(x.float(), w1.to(dt).float(), b1, padding=1)).to(dt).float()
    want = torch.cat([F.conv2d(hidden[:, 128 * k:128 * k + 128], w[k].to(dt).float(), b2[2 * k:2 * k + 2], padding=1)
                      for k in range(4)], 1)
    tol = 2e-2 if dt == torch.float16 else 1.5e-1
    assert y.shape == want.shape and (y.float() - want).abs().max() < tol
    assert torch.equal(db.heads_fused(x, t1, b1, f2, b2), y)
