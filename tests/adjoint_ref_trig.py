"""tests/adjoint_ref.py extended by the backward rules of sin, cos and log (include/flowz_hip.h, fz_run_block_grad):

    SIN  abar += g * cos(a)        COS  abar -= g * sin(a)        LOG  abar += g / a

cos(a) / sin(a) are the library's own functions (tests/fn_ref_trig.py) on the operand's forward value; each contribution is formed, then
added -- one float32 rounding each.  adjoint_ref.grad skips node kinds it does not know, so grad() below is a loop of its own in the same
documented order; on a graph without the three kinds it gives adjoint_ref.grad's bits.  Importing this module registers the forward
functions in adjoint_ref._UN (Layout.values and the reachability walk then know the kinds) and, through fn_ref_trig, in fn_ref.
"""
import numpy as np

import adjoint_ref as A
import fn_ref_trig as RT

F32, F64 = np.float32, np.float64
NEG0 = A.NEG0
A._UN.update({"sin": RT.sin, "cos": RT.cos, "log": RT.log})
Layout = A.Layout
forward = A.forward
rel_err = A.rel_err


def grad(prog, x, out_grad, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None, consts=None):
    """dict x / state / params / consts of fz_run_block_grad's bits (params / consts ADDED to accum_*, else from +0)"""
    L = Layout(prog)
    x = np.asarray(x, F32)
    yb = np.asarray(out_grad, F32)
    T, ns, _ = x.shape
    s = np.zeros((L.n_state, ns), F32) if state is None else np.array(state, F32)[:L.n_state].copy()
    c = L.consts if consts is None else np.asarray(consts, F32)
    S = np.empty((T, L.n_state, ns), F32)
    for t in range(T):
        S[t] = s
        s = L.next_state(L.values(x[t], s, params, c), s)
    Rs = np.zeros((L.n_state, ns), F32) if state_grad is None else np.array(state_grad, F32)[:L.n_state].copy()
    pb = np.zeros((L.n_param, ns), F32) if accum_params is None else np.array(accum_params, F32)[:L.n_param].copy()
    cb = np.zeros((L.n_const, ns), F32) if accum_consts is None else np.array(accum_consts, F32)[:L.n_const].copy()
    xb = np.empty((T, ns, L.n_in), F32)
    n = len(L.ir)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            v = L.values(x[t], S[t], params, c)
            g = [np.full(ns, NEG0, F32) for _ in range(n)]
            for j, o in enumerate(L.outs):                            # 1. output slots
                g[o] = g[o] + yb[t, :, j]
            for src, depth, r0 in L.lines:                            # 2. the pending line adjoint, then the shift
                g[src] = g[src] + Rs[r0]
                Rs[r0:r0 + depth - 1] = Rs[r0 + 1:r0 + depth].copy()
                Rs[r0 + depth - 1] = NEG0
            for k in range(n - 1, -1, -1):                            # 3. consumers in decreasing node order
                if not L.has[k]:
                    continue
                kind, a, b, _ = L.ir[k]
                gk = g[k]
                if kind == "const": cb[a] = cb[a] + gk
                elif kind == "param": pb[a] = pb[a] + gk
                elif kind == "delay":
                    r = L.row0[a] + b - 1
                    Rs[r] = Rs[r] + gk
                elif kind == "add":
                    g[a] = g[a] + gk
                    g[b] = g[b] + gk
                elif kind == "sub":
                    g[a] = g[a] + gk
                    g[b] = g[b] - gk
                elif kind == "mul":
                    g[a] = g[a] + gk * v[b]
                    g[b] = g[b] + gk * v[a]
                elif kind == "div":
                    q = gk / v[b]
                    g[a] = g[a] + q
                    g[b] = g[b] - q * v[k]
                elif kind == "neg": g[a] = g[a] - gk
                elif kind == "sqrt": g[a] = g[a] + gk * (F32(0.5) / v[k])
                elif kind == "exp": g[a] = g[a] + gk * v[k]
                elif kind == "tanh": g[a] = g[a] + gk * (F32(1) - v[k] * v[k])
                elif kind == "sin": g[a] = g[a] + gk * RT.cos(v[a])
                elif kind == "cos": g[a] = g[a] - gk * RT.sin(v[a])
                elif kind == "log": g[a] = g[a] + gk / v[a]
                elif kind == "abs": g[a] = np.where(v[a] > 0, g[a] + gk, np.where(v[a] < 0, g[a] - gk, g[a]))
                elif kind in ("min", "max"):
                    m = (v[b] < v[a]) if kind == "min" else (v[a] < v[b])
                    g[a] = np.where(m, g[a], g[a] + gk)
                    g[b] = np.where(m, g[b] + gk, g[b])
            for w in range(L.n_in):                                   # 4. the row's input adjoints
                acc = None
                for i, (kind, a, _, _) in enumerate(L.ir):
                    if kind == "input" and a == w and L.has[i]:
                        acc = g[i] if acc is None else acc + g[i]
                xb[t, :, w] = np.zeros(ns, F32) if acc is None else acc
    return {"x": xb, "state": Rs, "params": pb, "consts": cb}


def torch_forward(L, x, s0, p, c):
    """adjoint_ref.torch_forward with torch.sin / torch.cos / torch.log for the three kinds (exact functions, float64)"""
    import torch

    T = x.shape[0]
    rows = [s0[r] for r in range(L.n_state)]
    ys = []
    un = {"neg": torch.neg, "abs": torch.abs, "sqrt": torch.sqrt, "exp": torch.exp, "tanh": torch.tanh, "sin": torch.sin, "cos": torch.cos,
          "log": torch.log}
    for t in range(T):
        v = [None] * len(L.ir)
        for i, (kind, a, b, _) in enumerate(L.ir):
            if kind == "input": r = x[t, :, a]
            elif kind == "const": r = c[a]
            elif kind == "param": r = p[a]
            elif kind == "delay": r = rows[L.row0[a] + b - 1]
            elif kind == "add": r = v[a] + v[b]
            elif kind == "sub": r = v[a] - v[b]
            elif kind == "mul": r = v[a] * v[b]
            elif kind == "div": r = v[a] / v[b]
            elif kind in un: r = un[kind](v[a])
            elif kind == "min": r = torch.where(v[b] < v[a], v[b], v[a])
            elif kind == "max": r = torch.where(v[a] < v[b], v[b], v[a])
            elif kind in A._CMP: r = getattr(torch, kind)(v[a].detach(), v[b].detach()).to(x.dtype)
            else:
                raise NotImplementedError(kind)
            v[i] = r
        ys.append(torch.stack([v[o] for o in L.outs], -1))
        new = list(rows)
        for src, depth, r0 in L.lines:
            new[r0] = v[src]
            for a_ in range(1, depth):
                new[r0 + a_] = rows[r0 + a_ - 1]
        rows = new
    sT = torch.stack(rows) if rows else s0
    return torch.stack(ys), sT


def torch_grad(prog, x, out_grad, state, params, state_grad):
    """float64 autograd of the torch restatement: dict x / state / params / consts (numpy float64)"""
    import torch

    L = Layout(prog)
    ns = x.shape[1]
    t = lambda a, shape: torch.tensor(np.asarray(a, F64).reshape(shape), dtype=torch.float64, requires_grad=True)   # noqa: E731
    xt = t(x, x.shape)
    s0 = t(state if state is not None else np.zeros((L.n_state, ns)), (L.n_state, ns))
    p = t(params if params is not None else np.zeros((L.n_param, ns)), (L.n_param, ns))
    c = t(np.repeat(L.consts.astype(F64)[:, None], ns, 1), (L.n_const, ns))
    y, sT = torch_forward(L, xt, s0, p, c)
    loss = (y * torch.tensor(np.asarray(out_grad, F64))).sum()
    if state_grad is not None and L.n_state:
        loss = loss + (sT * torch.tensor(np.asarray(state_grad, F64))).sum()
    gx, gs, gp, gc = torch.autograd.grad(loss, (xt, s0, p, c), allow_unused=True)
    z = lambda gr, like: np.zeros(like.shape) if gr is None else gr.detach().numpy()   # noqa: E731
    return {"x": z(gx, xt), "state": z(gs, s0), "params": z(gp, p), "consts": z(gc, c)}
