"""float64 CPU reference of the per-range optimizer step (nmh_grad_sqnorm_ranges, nmh_clip_coef, nmh_adamw_step_ranges; trainer.FusedAdamW(ranges=)):
torch.optim.AdamW with ONE PARAM GROUP PER RANGE (lr * lr_scale, weight_decay * wd_scale) and clip_grad_norm_ over the groups' parameters.  A frozen range
(lr_scale 0) is simply not given to the optimizer and not to the clip: it is a parameter without a gradient."""
import torch


class RangedAdamWRef:
    """RangedAdamWRef(p0, bounds, scales, weight_decay, betas, eps, max_norm): p0 a flat tensor, bounds [R+1], scales [R][2].  step(g, lr, beta1=None) -> the
    clip's total norm (float); `flat()` -> the current parameters as one float64 vector; `frozen` -> bool mask over the elements."""

    def __init__(self, p0, bounds, scales, weight_decay, betas=(0.9, 0.999), eps=1e-8, max_norm=0.1):
        self.bounds, self.scales, self.max_norm = [int(b) for b in bounds], [(float(a), float(b)) for a, b in scales], max_norm
        assert len(self.bounds) == len(self.scales) + 1 and self.bounds[0] == 0 and self.bounds[-1] == p0.numel()
        p0 = p0.detach().cpu().double().reshape(-1)
        self.parts = [p0[lo:hi].clone().requires_grad_(ls != 0.0) for (lo, hi), (ls, _) in zip(zip(self.bounds[:-1], self.bounds[1:]), self.scales)]
        self.live = [r for r, (ls, _) in enumerate(self.scales) if ls != 0.0]
        self.opt = torch.optim.AdamW([{"params": [self.parts[r]], "lr": 0.0, "weight_decay": weight_decay * self.scales[r][1]} for r in self.live],
                                     lr=0.0, betas=tuple(betas), eps=eps)
        self.frozen = torch.zeros(p0.numel(), dtype=torch.bool)
        for r, (ls, _) in enumerate(self.scales):
            if ls == 0.0:
                self.frozen[self.bounds[r]:self.bounds[r + 1]] = True

    def step(self, g, lr, beta1=None):
        g = g.detach().cpu().double().reshape(-1)
        for group, r in zip(self.opt.param_groups, self.live):
            group["lr"] = lr * self.scales[r][0]
            if beta1 is not None:
                group["betas"] = (beta1, group["betas"][1])
            self.parts[r].grad = g[self.bounds[r]:self.bounds[r + 1]].clone()
        norm = torch.nn.utils.clip_grad_norm_([self.parts[r] for r in self.live], self.max_norm)
        self.opt.step()
        return float(norm)

    def flat(self):
        return torch.cat([p.detach() for p in self.parts])
