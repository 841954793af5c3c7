"""CPU: the float64 references of tests/_heads_ref.py are themselves checked, before tests/test_head_kernels_gpu.py holds the kernels of csrc/heads.hip to
them: the nearest-neighbour index map against its closed form, the adjoint against the forward by <fwd(y), d> == <y, adj(d)>, both losses against the fp32
oracle (oracle/heads_oracle.py, itself pinned to the reference classes by golden g15) and a hand-computed case, and every masked-CE case of the GPU test
against three wrong variants of the loss that a bound of CE_TOL_CEILING must tell apart."""
import math
import types

import pytest
import torch

from oracle import heads_oracle as HO
from oracle.gen_golden_heads import K, R, RO, class_weights, sem_labels, sr_targets
from oracle.mae3d_oracle import pad_grid
from tests import _heads_ref as HR

F64 = torch.float64


@pytest.mark.parametrize("R_,scale,Ro,copies", [(32, 1.6, 51, (1, 2)), (160, 1.6, 256, (1, 2)), (160, 2.4, 384, (2, 3)), (32, 2.4, 76, (1, 3)),
                                                (40, 1.6, 64, (1, 2)), (20, 2.4, 48, (2, 3))])
def test_nn_src_index_matches_closed_form(R_, scale, Ro, copies):
    """ATen's map == min(floor(d * float32(1 / scale)), R - 1); the clamp never acts when Ro = int(R * scale); copies per source index as listed"""
    ro, src = HR.nn_src_index(R_, scale)
    assert ro == Ro == int(R_ * scale)
    inv = torch.tensor(1.0 / scale, dtype=torch.float32)
    raw = (torch.arange(Ro, dtype=torch.float32) * inv).floor().long()
    assert torch.equal(src, raw.clamp(max=R_ - 1))
    assert int(raw.max()) == R_ - 1                       # the unclamped index already stays inside the source
    cnt = torch.bincount(src, minlength=R_)
    assert (int(cnt.min()), int(cnt.max())) == copies
    assert (R_, scale) in HR.NN_PAIRS


@pytest.mark.parametrize("R_,scale,Co,Cp,B", [(32, 1.6, 4, 8, 2), (32, 2.4, 19, 24, 1), (20, 2.4, 1, 8, 2), (40, 1.6, 32, 32, 1)])
def test_upsample_adjoint_is_the_transpose_of_upsample_fwd(R_, scale, Co, Cp, B):
    Ro, src = HR.nn_src_index(R_, scale)
    g = torch.Generator().manual_seed(R_ + Co)
    y = torch.randn((B * R_ ** 3, Cp), generator=g, dtype=F64)
    d = torch.randn((B, Co, Ro, Ro, Ro), generator=g, dtype=F64)
    up, adj = HR.upsample_fwd(y, Co, B, R_, src), HR.upsample_adjoint(d, Cp, R_, src)
    assert tuple(up.shape) == (B, Co, Ro, Ro, Ro) and tuple(adj.shape) == (B * R_ ** 3, Cp)
    lhs, rhs = (up * d).sum().item(), (y * adj).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert (adj[:, Co:] == 0).all()
    # the forward is F.interpolate itself
    ref = torch.nn.functional.interpolate(y.view(B, R_, R_, R_, Cp)[..., :Co].permute(0, 4, 1, 2, 3), scale_factor=scale, mode="nearest")
    assert torch.equal(up, ref)


def test_sr_loss_matches_the_oracle():
    tg = sr_targets()
    tgt = torch.cat([pad_grid(t, RO)[0] for t in tg])
    pred = torch.randn((2, 4, RO, RO, RO), generator=torch.Generator().manual_seed(1), requires_grad=True)
    stub = types.SimpleNamespace(output_resolution=RO)
    lo = HO.VoxelSROracle.forward_loss(stub, tg, pred)
    lo.backward()
    s0, s1, loss = HR.sr_loss(pred.detach(), tgt)
    assert s1.item() == (tgt[:, 3] > 0.01).sum().item() > 0
    assert abs(loss.item() - lo.item()) <= 1e-6 * abs(lo.item())
    for gs in (1.0, 0.37):
        gr = HR.sr_loss_grad(pred.detach(), tgt, gs)
        assert (gr - gs * pred.grad.double()).abs().max().item() <= 1e-6 * gr.abs().max().item()
        assert (gr[:, 3] == 0).all() and (gr[:, :3][(tgt[:, 3:] <= 0.01).expand(-1, 3, -1, -1, -1)] == 0).all()


def test_sr_loss_threshold_is_strict_at_float32_0p01():
    t = torch.zeros((1, 4, 1, 1, 3))
    t[0, 3, 0, 0] = torch.tensor([0.01, 0.0100001, 0.0099999])      # float32(0.01) itself is not counted
    p = torch.ones_like(t)
    s0, s1, _ = HR.sr_loss(p, t)
    assert s1.item() == 1.0 and s0.item() == 3.0


def test_masked_ce_matches_the_oracle():
    lab, cw = sem_labels(), class_weights()
    labels = torch.cat([pad_grid(t, R)[0] for t in lab])[:, 0]
    pred = (torch.randn((2, K, R, R, R), generator=torch.Generator().manual_seed(2)) * 2.0).requires_grad_(True)
    stub = types.SimpleNamespace(out_channels=K, input_resolution=R, class_weights=cw)
    lo, _, iou = HO.VoxelSemanticsOracle.forward_loss(stub, lab, pred)
    lo.backward()
    ref = HR.masked_ce(pred.detach(), labels, cw)
    assert abs(ref["ce"].item() - lo.item()) <= 1e-6 * abs(lo.item())
    assert abs(ref["miou"].item() - iou.item()) <= 1e-6 * abs(iou.item())
    assert abs((ref["sums"][0] / ref["sums"][1]).item() - ref["ce"].item()) <= 1e-14 * ref["ce"].item()
    gr = HR.masked_ce_grad(pred.detach(), labels, cw)
    assert (gr - pred.grad.double()).abs().max().item() <= 1e-6 * gr.abs().max().item()
    assert (gr.permute(0, 2, 3, 4, 1)[labels == 0] == 0).all()


def test_masked_ce_hand_computed_two_voxels():
    """K = 3; voxel 0 has label 2, voxel 1 is unlabelled: its logits count as (0, 0, 0) with target 0, so it adds cw[0] * log 3 to the numerator and cw[0] to
    the denominator; the soft IoU sees voxel 0 only, through the softmax of its raw logits"""
    a, cw = [0.5, -1.0, 2.0], [0.2, 0.7, 1.3]
    logits = torch.tensor([[a[0], 1.0], [a[1], 2.0], [a[2], 3.0]]).view(1, 3, 2, 1, 1)
    labels = torch.tensor([2.0, 0.0]).view(1, 2, 1, 1)
    z = sum(math.exp(v) for v in a)
    nll0 = math.log(z) - a[2]
    want_num, want_den = cw[2] * nll0 + cw[0] * math.log(3.0), cw[2] + cw[0]
    p1, p2 = math.exp(a[1]) / z, math.exp(a[2]) / z
    ref = HR.masked_ce(logits.double(), labels, torch.tensor(cw, dtype=F64))
    assert abs(ref["sums"][0].item() - want_num) < 1e-14 and abs(ref["sums"][1].item() - want_den) < 1e-14
    assert abs(ref["ce"].item() - want_num / want_den) < 1e-14
    want_iou = torch.tensor([[[p1, 0.0, 0.0], [p2, 1.0, p2]]], dtype=F64)
    assert (ref["iou"] - want_iou).abs().max().item() < 1e-15
    assert abs(ref["miou"].item() - 0.5 * (p2 / (p2 + 1.0 - p2 + 1e-8))) < 1e-15
    gr = HR.masked_ce_grad(logits.double(), labels, torch.tensor(cw, dtype=F64), 0.37)[0, :, :, 0, 0]
    want = [0.37 * cw[2] / want_den * (math.exp(a[k]) / z - (k == 2)) for k in range(3)]
    assert (gr[:, 0] - torch.tensor(want, dtype=F64)).abs().max().item() < 1e-15 and (gr[:, 1] == 0).all()
    # without class weights every voxel weighs 1: the denominator is the number of ALL voxels
    ref = HR.masked_ce(logits.double(), labels, None)
    assert abs(ref["ce"].item() - (nll0 + math.log(3.0)) / 2.0) < 1e-14 and ref["sums"][1].item() == 2.0


# ---- the GPU test's masked-CE cases tell wrong losses apart --------------------------------------------------------------------------------
def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("case", HR.ce_cases() + [HR.CE_FULL_SIZE], ids=lambda c: c[0])
def test_masked_ce_cases_discriminate_wrong_variants(case):
    """Three plausible wrong losses, computed here in float64 from the case's own inputs, against the reference.  A variant has to sit more than ten times
    the bound of the GPU test (the ceiling CE_TOL_CEILING any chosen bound stays under) away from the reference in a figure that test asserts:
      A. normalise by the number of labelled voxels instead of the weight sum over all voxels: moves ce and sums[1], scales the gradient;
      B. drop the cw[0] * log K of the unlabelled voxels from the numerator: moves ce and sums[0];
      C. soft IoU from the softmax of the MASKED logits (times the mask) instead of the raw ones.
    B coincides with the reference exactly when nothing is unlabelled (kind 'full', a case the kernel needs for its own sake), and so does A when there
    are no class weights either: asserted as such.  C is the reference for every input: the mask multiplies the probabilities
    afterwards, a labelled voxel's masked logits are its raw logits and an unlabelled voxel contributes 0 either way, so no test can tell C apart; asserted
    equal (to rounding) so that this stays a stated fact."""
    name, K_, has_cw, shape, B, sig, kind = case
    logits, labels, cw = HR.ce_inputs(case)
    ref = HR.masked_ce(logits, labels, cw)
    n_lab, n_unl = int((labels > 0).sum()), int((labels == 0).sum())
    cw0 = 1.0 if cw is None else float(cw[0].double())
    s0, s1, ce = ref["sums"][0].item(), ref["sums"][1].item(), ref["ce"].item()
    need = 10 * HR.CE_TOL_CEILING
    # the case is what it says it is
    assert n_lab > 0
    if kind == "full":
        assert n_unl == 0
    else:
        assert 0.3 < n_unl / labels.numel() < (0.65 if kind == "blank1" else 0.5)
    if kind == "absent3":
        assert int((labels[0] == 3).sum()) == 0 and int((labels[1] == 3).sum()) > 0 and ref["iou"][0, 2, 1].item() == 0.0
    if kind == "blank1":
        assert int((labels[1] > 0).sum()) == 0 and (ref["iou"][1] == 0).all()
    if has_cw:
        assert abs(cw0 - float(cw[1:].min())) > 0.4
    # A
    ce_a = s0 / n_lab
    if kind == "full" and not has_cw:
        assert ce_a == ce
    else:
        assert _rel(ce_a, ce) > need and _rel(float(n_lab), s1) > need       # the gradient of A is the reference's times s1 / n_lab
    # B
    s0_b = s0 - n_unl * cw0 * math.log(K_)
    if kind == "full":
        assert s0_b == s0
    else:
        assert _rel(s0_b, s0) > need and _rel(s0_b / s1, ce) > need
    # C
    if logits.numel() <= 32 ** 3 * 32:
        m = (labels > 0).double()[:, None]
        prob_c = torch.softmax(logits.double() * m, 1) * m
        prob = torch.softmax(logits.double(), 1) * m
        assert (prob_c - prob).abs().max().item() < 1e-15
