"""Plain torch references of the kept-token patch embed, from the definitions: the integer row map, the im2row index gather, and the
float64 LayerNorm -> + pos -> mask-token replacement with its autograd.  No kernel of the project is called here."""
import random

import torch
import torch.nn.functional as F

F64 = torch.float64


def rowmap_ref(mask, cap):
    """mask [n] uint8 (any non-zero value = removed) -> int32 [n + 2]: the compact row of every kept token in raster order (-1: removed, or no row left),
    the kept count clamped to cap, and the overflow flag"""
    kept = (mask.view(-1) == 0).to(torch.int64)
    r = torch.cumsum(kept, 0) - kept
    K = int(kept.sum())
    rm = torch.where((kept == 1) & (r < cap), r, torch.full_like(r, -1))
    return torch.cat([rm, torch.tensor([min(K, cap), int(K > cap)])]).to(torch.int32)


def masks_for(n, seed):
    """the masks of one token count: [(name, uint8 [n])].  i.i.d. Bernoulli at 0.75 for every n, and the block mask of the reference too where n is a cube with 4 | g"""
    from oracle import mae3d_oracle as O
    gen = torch.Generator().manual_seed(seed)
    g = round(n ** (1.0 / 3.0))
    drawn = [("bernoulli", (torch.rand(n, generator=gen) < 0.75).to(torch.uint8))]
    if g ** 3 == n and g % 4 == 0:
        drawn.append(("block", O.draw_block_mask((g, g, g), 0.75, rng=random.Random(seed)).to(torch.uint8).reshape(-1)))
    first, last = torch.ones(n, dtype=torch.uint8), torch.ones(n, dtype=torch.uint8)
    first[0], last[n - 1] = 0, 0
    odd = (torch.rand(n, generator=gen) < 0.75).to(torch.uint8)
    odd = odd * torch.where(torch.rand(n, generator=gen) < 0.5, 255, 2).to(torch.uint8)   # removed entries hold 255 or 2, never 1
    return drawn + [("all_removed", torch.ones(n, dtype=torch.uint8)), ("none_removed", torch.zeros(n, dtype=torch.uint8)), ("only_first", first),
            ("only_last", last), ("values_255_and_2", odd)]


def caps_for(n, K):
    """([caps the kept tokens fit into], [caps they overflow]); a capacity of zero is refused by the wrapper and is tested apart"""
    cand = [K, min(n, -(-K // 64) * 64), n, max(1, K - 1), 1]
    fit = sorted({c for c in cand if c >= max(K, 1)})
    over = sorted({c for c in cand if 1 <= c < K})
    return fit, over


def im2row_ref(x, dt):
    """x [B, 4, R, R, R] -> [B, g^3, 256] of dtype dt: row (z, y, x) holds x[b, ci, 4 z + kz, 4 y + ky, 4 x + kx] at column ci 64 + kz 16 + ky 4 + kx.
    Pure indexing and one cast (round to nearest even), on whatever device x lives on"""
    B, _, R = x.shape[0], x.shape[1], x.shape[2]
    g = R // 4
    return x.view(B, 4, g, 4, g, 4, g, 4).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, g ** 3, 256).to(dt)


def embed_post_ref(y_tok, gamma, beta, pos, mask, mask_token, eps=1e-5):
    """float64: y_tok [B, n, C] (one row per token; the rows of removed tokens may hold anything finite) -> tok [B, n, C], mean [B, n], rstd [B, n]"""
    C = y_tok.shape[-1]
    ln = F.layer_norm(y_tok, (C,), gamma, beta, eps) + pos
    tok = torch.where((mask != 0)[None, :, None], mask_token.view(1, 1, C).expand_as(ln), ln)
    mean = y_tok.mean(-1)
    rstd = (y_tok.var(-1, unbiased=False) + eps).rsqrt()
    return tok, mean, rstd


def scatter_rows(y_compact, rowmap, n, fill=0.0):
    """compact [B, cap, C] -> one row per token [B, n, C]: token t takes row rowmap[t]; tokens without a row take `fill`"""
    B, _, C = y_compact.shape
    rm = rowmap[:n].long()
    out = torch.full((B, n, C), fill, dtype=y_compact.dtype, device=y_compact.device)
    k = rm >= 0
    out[:, k] = y_compact[:, rm[k]]
    return out


def chain_ref(x, w, b, gamma, beta, pos, mask, mask_token, dtok):
    """float64 reference of the whole patch embed and its parameter gradients: F.conv3d(stride 4) -> LayerNorm -> + pos -> mask-token replacement, with
    upstream gradient dtok.  Every argument is float64 and holds the values the kernels see.  -> tok [B, n, C], (dW, db, dgamma, dbeta, dmask_token)"""
    ps = [t.clone().requires_grad_(True) for t in (w, b, gamma, beta, mask_token)]
    y = F.conv3d(x, ps[0], ps[1], stride=4)
    B, C = y.shape[0], y.shape[1]
    y_tok = y.flatten(2).transpose(1, 2)
    tok, _, _ = embed_post_ref(y_tok, ps[2], ps[3], pos, mask, ps[4])
    grads = torch.autograd.grad((tok * dtok.view(B, -1, C)).sum(), ps)
    return tok.detach(), grads
