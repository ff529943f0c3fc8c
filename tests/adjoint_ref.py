"""The backward of a block (fz_run_block_grad) restated in numpy float32, in the order include/flowz_hip.h documents; and a float64
torch restatement of the forward IR, for autograd and finite differences to check the restatement against.

The numpy restatement is vectorised over the streams and loops over the rows.  Every operation is one float32 operation of numpy
(IEEE, round to nearest, denormals kept), so it gives the adjoint kernel's bits: for every row t = T-1 .. 0 a node's adjoint starts
at -0.0 and receives (1) the out_grad of its output slots in slot order, (2) the pending line adjoint of the line it feeds, (3) its
consumers' contributions in decreasing node order (operand a first); DELAY / PARAM / CONST nodes then add their adjoint into the adjoint
state row / the parameter / the coefficient accumulator.  Nodes no adjoint reaches (only comparisons read them) contribute nothing.
Forward values are tests/fn_ref.py's (the kernels' own exp / tanh algorithm).
"""
import numpy as np

import fn_ref as R

F32, F64 = np.float32, np.float64
NEG0 = F32(-0.0)
_BIN = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "min": R.fmin, "max": R.fmax}
_UN = {"neg": np.negative, "abs": R.fabs, "sqrt": R.sqrt, "exp": R.exp, "tanh": R.tanh}
_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}


class Layout:
    """What the restatements need of a program: its IR, outputs, delay-line rows and current coefficients."""

    def __init__(self, prog):
        self.ir = prog.ir()
        self.outs = prog.outputs()
        self.lines = []                       # (src node, depth, first state row)
        r = 0
        for src, depth in prog.lines():
            self.lines.append((src, depth, r))
            r += depth
        self.row0 = {src: r0 for src, _, r0 in self.lines}
        self.n_state, self.n_in, self.n_out = r, prog.n_in, prog.n_out
        self.n_param, self.n_const = prog.n_param, prog.n_const
        self.consts = np.asarray(prog.consts(), F32)
        self.has = self._reached()

    def _reached(self):
        """per node: does any adjoint reach it (output slot, line source, or a consumer other than a comparison that is reached)"""
        has = [False] * len(self.ir)
        for o in self.outs:
            has[o] = True
        for src, _, _ in self.lines:
            has[src] = True
        for k in range(len(self.ir) - 1, -1, -1):
            kind, a, b, _ = self.ir[k]
            if not has[k]:
                continue
            if kind in ("add", "sub", "mul", "div", "min", "max"):
                has[a] = has[b] = True
            elif kind in _UN:
                has[a] = True
        return has

    def values(self, xt, s, params, consts):
        """node values of one row (float32 arrays over the streams): xt [ns, n_in], s [n_state, ns]"""
        ns = xt.shape[0]
        v = [None] * len(self.ir)
        with np.errstate(all="ignore"):
            for i, (kind, a, b, val) in enumerate(self.ir):
                if kind == "input": r = xt[:, a]
                elif kind == "const": r = np.full(ns, consts[a], F32)
                elif kind == "param": r = params[a]
                elif kind == "delay": r = s[self.row0[a] + b - 1]
                elif kind in _BIN: r = _BIN[kind](v[a], v[b])
                elif kind in _UN: r = _UN[kind](v[a])
                elif kind in _CMP: r = np.where(_CMP[kind](v[a], v[b]), F32(1), F32(0))
                else:
                    raise NotImplementedError(kind)
                v[i] = np.asarray(r, F32)
        return v

    def next_state(self, v, s):
        sn = np.empty_like(s)
        for src, depth, r0 in self.lines:
            sn[r0] = v[src]
            sn[r0 + 1:r0 + depth] = s[r0:r0 + depth - 1]
        return sn


def forward(prog, x, state=None, params=None, consts=None):
    """(y [T, ns, n_out], state after) of the block, float32 -- the forward kernels' bits"""
    L = Layout(prog)
    x = np.asarray(x, F32)
    T, ns, _ = x.shape
    s = np.zeros((L.n_state, ns), F32) if state is None else np.array(state, F32)[:L.n_state].copy()
    c = L.consts if consts is None else np.asarray(consts, F32)
    y = np.empty((T, ns, L.n_out), F32)
    for t in range(T):
        v = L.values(x[t], s, params, c)
        for j, o in enumerate(L.outs):
            y[t, :, j] = v[o]
        s = L.next_state(v, s)
    return y, s


def grad(prog, x, out_grad, state=None, params=None, state_grad=None, accum_params=None, accum_consts=None, consts=None):
    """dict x / state / params / consts of fz_run_block_grad's bits (params / consts ADDED to accum_*, else from +0)"""
    L = Layout(prog)
    x = np.asarray(x, F32)
    yb = np.asarray(out_grad, F32)
    T, ns, _ = x.shape
    s = np.zeros((L.n_state, ns), F32) if state is None else np.array(state, F32)[:L.n_state].copy()
    c = L.consts if consts is None else np.asarray(consts, F32)
    S = np.empty((T, L.n_state, ns), F32)                 # the state before every row
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
                elif kind == "abs": g[a] = np.where(v[a] > 0, g[a] + gk, np.where(v[a] < 0, g[a] - gk, g[a]))
                elif kind in ("min", "max"):
                    m = (v[b] < v[a]) if kind == "min" else (v[a] < v[b])
                    g[a] = np.where(m, g[a], g[a] + gk)
                    g[b] = np.where(m, g[b] + gk, g[b])
                # input: read below; comparisons: no arithmetic
            for w in range(L.n_in):                                   # 4. the row's input adjoints
                acc = None
                for i, (kind, a, _, _) in enumerate(L.ir):
                    if kind == "input" and a == w and L.has[i]:
                        acc = g[i] if acc is None else acc + g[i]
                xb[t, :, w] = np.zeros(ns, F32) if acc is None else acc
    return {"x": xb, "state": Rs, "params": pb, "consts": cb}


# ---- float64 torch restatement of the IR (autograd and finite differences check the numpy restatement with it) -------------------
def torch_forward(L, x, s0, p, c):
    """y [T, ns, n_out], s_T in the dtype of the arguments: x [T, ns, n_in], s0 [n_state, ns], p [n_param, ns], c [n_const, ns] (a
    coefficient per stream, so that its gradient is per stream).  Exact functions (torch.tanh, torch.exp) instead of the kernels'."""
    import torch

    T = x.shape[0]
    rows = [s0[r] for r in range(L.n_state)]
    ys = []
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
            elif kind == "neg": r = -v[a]
            elif kind == "abs": r = torch.abs(v[a])
            elif kind == "sqrt": r = torch.sqrt(v[a])
            elif kind == "exp": r = torch.exp(v[a])
            elif kind == "tanh": r = torch.tanh(v[a])
            elif kind == "min": r = torch.where(v[b] < v[a], v[b], v[a])
            elif kind == "max": r = torch.where(v[a] < v[b], v[b], v[a])
            elif kind in _CMP:
                r = getattr(torch, {"lt": "lt", "le": "le", "gt": "gt", "ge": "ge", "eq": "eq", "ne": "ne"}[kind])(v[a].detach(), v[b].detach()).to(x.dtype)
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


def torch_grad(prog, x, out_grad, state, params, state_grad, dtype=None):
    """float64 autograd of the torch restatement: dict x / state / params / consts (numpy float64)"""
    import torch

    dtype = dtype or torch.float64
    L = Layout(prog)
    ns = x.shape[1]
    t = lambda a, shape: torch.tensor(np.asarray(a, F64).reshape(shape), dtype=dtype, requires_grad=True)   # noqa: E731
    xt = t(x, x.shape)
    s0 = t(state if state is not None else np.zeros((L.n_state, ns)), (L.n_state, ns))
    p = t(params if params is not None else np.zeros((L.n_param, ns)), (L.n_param, ns))
    c = t(np.repeat(L.consts.astype(F64)[:, None], ns, 1), (L.n_const, ns))
    y, sT = torch_forward(L, xt, s0, p, c)
    loss = (y * torch.tensor(np.asarray(out_grad, F64), dtype=dtype)).sum()
    if state_grad is not None and L.n_state:
        loss = loss + (sT * torch.tensor(np.asarray(state_grad, F64), dtype=dtype)).sum()
    gx, gs, gp, gc = torch.autograd.grad(loss, (xt, s0, p, c), allow_unused=True)
    z = lambda gr, like: np.zeros(like.shape) if gr is None else gr.detach().numpy()   # noqa: E731
    return {"x": z(gx, xt), "state": z(gs, s0), "params": z(gp, p), "consts": z(gc, c)}


def rel_err(got, want):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    den = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / (den if den > 0 else 1.0))
