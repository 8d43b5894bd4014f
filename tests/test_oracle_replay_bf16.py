"""nca_oracle.cond_replay_vjp(bf16_operands=True) on the CPU: the replay VJP whose three matrix products take bf16 operands
(straight-through), i.e. cond_grow_bf16_loss_grads' step restarted from a recorded input.  On a history that cond_step_bf16 itself
produced the two are the same function, so the chained replay must equal autograd through cond_grow_bf16_loss_grads; with the flag
off nothing changes; and the two operand precisions differ by the few per cent the bf16 bounds of the GPU tests allow for."""
import torch

from oracle import nca_oracle as O
from test_oracle_replay import rand_cond_prm

F64 = torch.float64


def bf16_history(B=2, C=12, H=10, W=12, gch=8, Tn=3, seed=3):
    """a float64 history of bf16-representable states in the kernels' layout, stepped by cond_step_bf16, alpha evolving"""
    gen = torch.Generator().manual_seed(seed)
    prm = {k: v.double() for k, v in rand_cond_prm(C, seed=seed, out_scale=1.0).items()}
    x0 = O._bf(torch.rand(B, C, H, W, generator=gen).double())
    x0[:, 3] = O._bf(x0[:, 3] * 0.12)
    gpad = O.cond_pad_goal(O._bf(torch.randn(B, gch, H, W, generator=gen).double() * 0.5), C)
    us = [torch.rand(B, 1, H, W, generator=gen) for _ in range(Tn)]
    cot = torch.randn(B, C, H, W, generator=gen).double()
    states, pre, x = [x0], [torch.zeros(B, H, W, dtype=torch.uint8)], x0
    with torch.no_grad():
        for u in us:
            x, p, pend = O.cond_step_bf16(x, gpad, u, prm)
            states.append(pend)
            pre.append(p[:, 0].to(torch.uint8))
    return prm, x0, gpad, us, cot, torch.stack(states), torch.stack(pre)


def _worst(a, b):
    ga = {"x0": a[0], "goal": a[1], **a[2]}
    gb = {"x0": b[0], "goal": b[1], **b[2]}
    return {k: float((ga[k] - gb[k]).norm() / gb[k].norm().clamp_min(1e-300)) for k in ga}


def test_bf16_operand_replay_equals_autograd():
    prm, x0, gpad, us, cot, states, pre = bf16_history()
    assert 0.05 < float(pre[1:].float().mean()) < 0.999           # life masks that evolve
    got = O.cond_replay_vjp(states, pre, gpad, us, prm, cot, 3, bf16_operands=True)
    _, gx, gg, gw = O.cond_grow_bf16_loss_grads(x0, gpad, us, prm, 3, 0.1, 0.5, cot)
    e = _worst(got, (gx, gg, gw))
    assert got[0].dtype == F64 and max(e.values()) < 1e-10, e


def test_flag_off_is_the_exact_replay_and_differs_by_the_bf16_budget():
    prm, x0, gpad, us, cot, states, pre = bf16_history(seed=4)
    exact = O.cond_replay_vjp(states, pre, gpad, us, prm, cot, 3)
    again = O.cond_replay_vjp(states, pre, gpad, us, prm, cot, 3, bf16_operands=False)
    assert all(v == 0.0 for v in _worst(again, exact).values())
    e = _worst(O.cond_replay_vjp(states, pre, gpad, us, prm, cot, 3, bf16_operands=True), exact)
    print(f"\n[oracle] bf16-operand replay VJP vs exact-product replay VJP, relative L2: {e}")
    assert 1e-4 < max(e.values()) < 8e-2, e
