"""What the eager-launched fused sampling loops share (DPMSolverPP._multistep_fused, SpacedDiffusion._loop_fused,
SASolver._pec_fused): the
device coefficient table and the loop that puts one fused launch behind each model call."""
from __future__ import annotations


def device_table(cache: dict, key, build_rows, dev, n):
    """(coefficient table, its T_NEXT column - the model-input time of the forward that follows each row - as
    [steps, 2n]) on the device ``dev``; ``build_rows()`` gives the host table.  Kept in ``cache`` under ``key``, so that
    the next loop with the same configuration uploads nothing."""
    from .._lib import DPMPP_T_NEXT as T_NEXT         # == DDPM_T_NEXT == SA_T_NEXT: the same column of every row layout
    hit = cache.get(key)
    if hit is None:
        rows = build_rows()
        t_next = rows[:, T_NEXT][:, None].expand(rows.shape[0], 2 * n).contiguous()
        # pinned and non-blocking: a pageable upload makes the host wait for the forward that is already queued
        hit = tuple(t.pin_memory().to(dev, non_blocking=True) for t in (rows, t_next))
        if len(cache) >= 8:
            cache.clear()
        cache[key] = hit
    return hit


def fused_loop(steps, x, xm, t, forward, table, step):
    """``steps`` times {eps = forward(xm, t); x = step(k, eps, x, rows)}, the time of the next forward read from the
    table.  ``table(eps, x)`` is asked once, after the first forward: None when the kernel does not take this model
    output, else (rows, t_next) on the device.  Returns (x, None), or (None, eps) after that None: the caller goes on
    eagerly from the first model output."""
    for k in range(steps):
        eps = forward(xm, t)
        if k == 0:
            # the table is built (host work) and uploaded behind the first forward's launches, not in front of them
            hit = table(eps, x)
            if hit is None:
                return None, eps
            rows, t_next = hit
        x = step(k, eps, x, rows)
        t = t_next[k]
    return x, None
