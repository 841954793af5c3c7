"""Gradient accumulation, the host arithmetic: trainer.accum_epoch_plan, which both epoch loops cut their optimizer steps with, and the
size of the OneCycle schedule of an accumulated run.  The step itself is tests/test_accumulate_gpu.py."""
import math

import pytest


@pytest.mark.parametrize("k", [1, 2, 3, 7, 8])
def test_accum_epoch_plan_groups_in_order_and_only_the_last_step_is_short(k):
    from nerf_mae_amd.trainer import accum_epoch_plan
    batches = [[2 * i, 2 * i + 1] for i in range(7)]
    plan = accum_epoch_plan(batches, k)
    assert len(plan) == math.ceil(7 / k)
    assert all(len(step) == k for step in plan[:-1])
    assert 1 <= len(plan[-1]) <= k and len(plan[-1]) == 7 - k * (len(plan) - 1)
    assert [b for step in plan for b in step] == batches           # every batch once, in the epoch's order
    assert accum_epoch_plan(iter(batches), k) == plan              # any iterable


def test_accum_epoch_plan_refuses_k_below_one_and_takes_an_empty_epoch():
    from nerf_mae_amd.trainer import accum_epoch_plan
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError):
            accum_epoch_plan([[0]], k)
    assert accum_epoch_plan([], 3) == []


@pytest.mark.parametrize("n,batch,world,k,epochs", [(5, 1, 1, 2, 1), (7, 1, 1, 3, 4), (9, 2, 2, 2, 3), (4, 4, 1, 8, 2)])
def test_onecycle_of_an_accumulated_run_counts_optimizer_steps(n, batch, world, k, epochs):
    """the schedule is stepped once per optimizer step: its length is epochs * ceil(micro_steps / k), the same on every rank, and its last step is the last
    optimizer step of the run"""
    from nerf_mae_amd.trainer import OneCycle, accum_epoch_plan, dp_epoch_plan
    totals = []
    for rank in range(world):
        micro = dp_epoch_plan(n, batch, rank, world, 0)
        steps = accum_epoch_plan(micro, k)
        totals.append(OneCycle(1e-3, epochs * len(steps)).total)
        assert totals[-1] == epochs * math.ceil(len(micro) / k)
        assert [len(s) for s in steps] == [len(s) for s in accum_epoch_plan(dp_epoch_plan(n, batch, 0, world, 0), k)]      # the data-parallel invariant
    assert len(set(totals)) == 1
    sch = OneCycle(1e-3, totals[0])
    lr_last, _ = sch.at(totals[0] - 1)
    assert lr_last == pytest.approx(sch.min_lr)


def test_resume_section_records_accumulate_and_another_k_is_refused():
    """restore_resume's refusal, on host stand-ins: the section carries k only when it is not 1, and a file written under another k does not load"""
    import torch
    from nerf_mae_amd.trainer import restore_resume, resume_section

    class Model:
        _offsets = {}

        def named_parameters(self):
            return []

    class Opt:
        def __init__(self, k):
            self.m, self.v, self.t, self.lr, self.betas, self.accumulate = torch.zeros(4), torch.zeros(4), 3, 1e-3, (0.9, 0.999), k

    assert "accumulate" not in resume_section(Model(), Opt(1), 3)
    sec = resume_section(Model(), Opt(2), 3)
    assert sec["accumulate"] == 2
    restore_resume(sec, Model(), Opt(2), "test")
    with pytest.raises(RuntimeError, match="accumulate"):
        restore_resume(sec, Model(), Opt(1), "test")
    with pytest.raises(RuntimeError, match="accumulate"):
        restore_resume(resume_section(Model(), Opt(1), 3), Model(), Opt(3), "test")
