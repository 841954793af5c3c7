"""float64 restatements of the operations behind csrc/heads.hip, in plain torch, written from the definition of each operation (nn.Upsample(nearest),
the masked RGB MSE, nn.CrossEntropyLoss(weight) on masked logits + the soft-IoU sums, UnetResBlock, a 1x1x1 conv) and not from the kernels' loops.
tests/test_heads_ref_cpu.py checks these references themselves (against ATen, against each other as adjoints, against oracle/heads_oracle.py and a hand
computed case); tests/test_head_kernels_gpu.py checks every kernel against them.  The functions run on whatever device their inputs live on: the CPU by
default, the HIP device for the full-size cases, where only torch indexing / index_add_ are used (never the kernels under test)."""
import torch
import torch.nn.functional as F

F64 = torch.float64
NN_PAIRS = [(32, 1.6), (160, 1.6), (160, 2.4), (32, 2.4), (40, 1.6), (20, 2.4)]   # (R, scale) -> Ro = 51, 256, 384, 76, 64, 48
CE_TOL_CEILING = 2e-5   # no bound of the masked-CE kernel tests may exceed this (relative; of max|ref| for the gradient)


# ---- nearest upsampling --------------------------------------------------------------------------------------------------------------------
def nn_src_index(R, scale):
    """(Ro, src): ATen's own answer to `which source index does output index d read`, from F.interpolate on a ramp"""
    ramp = torch.arange(R, dtype=torch.float32).view(1, 1, R, 1, 1)
    up = F.interpolate(ramp, scale_factor=scale, mode="nearest")[0, 0, :, 0, 0]
    return int(up.numel()), up.round().long()


def inv_scale_f32(scale):
    """the fp32 value of 1 / scale that the head passes to the kernels"""
    return float(torch.tensor(1.0 / scale, dtype=torch.float32))


def upsample_fwd(y, Co, B, R, src):
    """channels-last y [B*R^3][Cp] -> (B,Co,Ro,Ro,Ro) in y's dtype: pure copies"""
    src = src.to(y.device)
    t = y.view(B, R, R, R, -1)[..., :Co].permute(0, 4, 1, 2, 3)
    return t[:, :, src][:, :, :, src][:, :, :, :, src].contiguous()


def upsample_adjoint(dpred, Cp, R, src):
    """float64 transpose of upsample_fwd: (B,Co,Ro,Ro,Ro) -> [B*R^3][Cp], columns >= Co zero"""
    src = src.to(dpred.device)
    B, Co = dpred.shape[:2]
    t = dpred.to(F64)
    for dim in (4, 3, 2):
        shape = list(t.shape)
        shape[dim] = R
        t = torch.zeros(shape, dtype=F64, device=t.device).index_add_(dim, src, t)
    out = torch.zeros((B, R, R, R, Cp), dtype=F64, device=t.device)
    out[..., :Co] = t.permute(0, 2, 3, 4, 1)
    return out.view(B * R ** 3, Cp)


# ---- VoxelSR loss --------------------------------------------------------------------------------------------------------------------------
def sr_loss(pred, tgt):
    """pred, tgt (B,4,...) -> (sum m |p_rgb - t_rgb|^2, sum m, their ratio) in float64, m = t_alpha > 0.01 (strict)"""
    p, t = pred.to(F64).permute(0, 2, 3, 4, 1), tgt.to(F64).permute(0, 2, 3, 4, 1)
    m = (t[..., 3:] > 0.01).to(F64)
    s0, s1 = (((p[..., :3] - t[..., :3]) ** 2) * m).sum(), m.sum()
    return s0, s1, s0 / s1


def sr_loss_grad(pred, tgt, gscale=1.0):
    """d(gscale * loss) / d pred, closed form: 2 gscale m (p - t) / sum m on the RGB planes, 0 on the alpha plane"""
    p, t = pred.to(F64), tgt.to(F64)
    m = (t[:, 3:] > 0.01).to(F64)
    g = torch.zeros_like(p)
    g[:, :3] = 2.0 * gscale * m * (p[:, :3] - t[:, :3]) / m.sum()
    return g


# ---- VoxelSemantics loss -------------------------------------------------------------------------------------------------------------------
def masked_ce(logits, labels, cw):
    """logits (B,K,*), labels (B,*) class ids with 0 = unlabelled, cw [K] or None -> dict in float64:
    sums = [sum_v w nll, sum_v w], ce = their ratio, iou [B][K-1][3] = {sum_v m p_k, #(label == k), sum_{label == k} p_k}, miou"""
    B, K = logits.shape[:2]
    p = logits.to(F64).reshape(B, K, -1).permute(0, 2, 1)           # (B,V,K)
    t = labels.reshape(B, -1).long()
    m = (t > 0)
    pm, tm = p * m[..., None].to(F64), t * m
    w = None if cw is None else cw.to(F64)
    ce = F.cross_entropy(pm.reshape(-1, K), tm.reshape(-1), weight=w)
    nll = F.cross_entropy(pm.reshape(-1, K), tm.reshape(-1), weight=w, reduction="sum")
    wsum = float(t.numel()) if w is None else w[tm.reshape(-1)].sum()
    prob = F.softmax(p, dim=-1) * m[..., None].to(F64)               # the softmax of the RAW logits, masked afterwards
    onehot = torch.zeros_like(prob).scatter_(-1, tm[..., None], 1.0)
    pk, ok = prob[..., 1:], onehot[..., 1:]
    inter, cnt, sp = (pk * ok).sum(1), ok.sum(1), pk.sum(1)
    union = (pk + ok - pk * ok).sum(1)
    miou = (inter / (union + 1e-8)).mean()
    return dict(ce=ce, sums=torch.stack([nll, torch.as_tensor(wsum, dtype=F64)]), iou=torch.stack([sp, cnt, inter], -1), miou=miou)


def masked_ce_grad(logits, labels, cw, gscale=1.0):
    """d(gscale * ce) / d logits by float64 autograd"""
    x = logits.detach().to(F64).requires_grad_(True)
    (masked_ce(x, labels, cw)["ce"] * gscale).backward()
    return x.grad


def ce_cases():
    """the masked-CE cases of the GPU test, shared with the CPU test that shows each of them tells the wrong variants apart.
    (name, K, class weights?, spatial shape, B, logit sigma, kind); kind: 'mixed' = ~40 % unlabelled, 'absent3' = class 3 absent from sample 0,
    'blank1' = sample 1 entirely unlabelled, 'full' = no unlabelled voxel"""
    cs = []
    for K in (2, 5, 19, 32):
        for cw in (False, True):
            for sig in (1.0, 4.0):
                shape, B = ((7, 7, 7), 3) if (K + cw + int(sig)) % 2 else ((32, 32, 32), 1)
                cs.append((f"K{K}-{'cw' if cw else 'nocw'}-s{sig:g}-V{shape[0]}-B{B}", K, cw, shape, B, sig, "mixed"))
    cs.append(("K19-cw-s4-V32-B3", 19, True, (32, 32, 32), 3, 4.0, "mixed"))
    cs.append(("K5-nocw-s1-V7-B1", 5, False, (7, 7, 7), 1, 1.0, "mixed"))
    cs.append(("K5-cw-s4-V7-B3-absent3", 5, True, (7, 7, 7), 3, 4.0, "absent3"))
    cs.append(("K19-cw-s1-V32-B3-blank1", 19, True, (32, 32, 32), 3, 1.0, "blank1"))
    cs.append(("K19-cw-s4-V7-B3-full", 19, True, (7, 7, 7), 3, 4.0, "full"))
    return cs


CE_FULL_SIZE = ("K19-cw-s4-V160-B1", 19, True, (160, 160, 160), 1, 4.0, "mixed")


def ce_inputs(case):
    """(logits fp32 (B,K,*shape), labels fp32 (B,*shape), cw fp32 [K] or None) of a case, on the CPU"""
    name, K, has_cw, shape, B, sig, kind = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    logits = torch.randn((B, K) + tuple(shape), generator=g) * sig
    labels = torch.randint(1, K, (B,) + tuple(shape), generator=g).float()
    if kind != "full":
        labels[torch.rand(labels.shape, generator=g) < 0.4] = 0.0
    if kind == "absent3":
        labels[0][labels[0] == 3] = 1.0
    if kind == "blank1":
        labels[1] = 0.0
    cw = None
    if has_cw:   # cw[0] clearly different from the rest: the unlabelled voxels weigh 0.05, the classes 0.5 .. 1.5
        cw = torch.cat([torch.tensor([0.05]), 0.5 + torch.rand(K - 1, generator=g)])
    return logits, labels, cw


# ---- encoder1 and the output conv ----------------------------------------------------------------------------------------------------------
def _inorm(t):
    mu = t.mean((2, 3, 4), keepdim=True)
    var = ((t - mu) ** 2).mean((2, 3, 4), keepdim=True)
    return (t - mu) / torch.sqrt(var + 1e-5)


def _lrelu(pre, slope, sign):
    """LeakyReLU; with `sign` (bool, pre's shape) the slope of every element is chosen by it instead of by pre's own sign (value and derivative)"""
    return F.leaky_relu(pre, slope) if sign is None else pre * torch.where(sign, torch.ones((), dtype=pre.dtype), torch.full((), slope, dtype=pre.dtype))


def res_block(x, w1, b1, w2, b2, w3, b3, slope=0.01, signs=None):
    """UnetResBlock(4 -> C) (unetr_block.py:23-71) in the dtype of its arguments: lrelu(IN(conv2(lrelu(IN(conv1 x)))) + IN(conv3 x)), affine-free
    InstanceNorm with eps 1e-5 and biased variance; x (B,4,S,S,S), w1 (C,4,3,3,3), w2 (C,C,3,3,3), w3 (C,4,1,1,1).  signs = (s1, s2): returns
    (out, (pre1, pre2)) with the branch of the two LeakyReLUs given by s1 / s2 (the signs an implementation stored), pre1 / pre2 their float64 arguments"""
    pre1 = _inorm(F.conv3d(x, w1, b1, padding=1))
    o = _inorm(F.conv3d(_lrelu(pre1, slope, None if signs is None else signs[0]), w2, b2, padding=1))
    pre2 = o + _inorm(F.conv3d(x, w3, b3))
    out = _lrelu(pre2, slope, None if signs is None else signs[1])
    return out if signs is None else (out, (pre1.detach(), pre2.detach()))


def out_conv_upsample(d0, w, b, B, R, src):
    """1x1x1 conv on channels-last d0 [B*R^3][C] with w (Co,C), b (Co) followed by nearest upsampling -> (B,Co,Ro,Ro,Ro)"""
    y = d0 @ w.t() + b
    return upsample_fwd(y, w.shape[0], B, R, src)
