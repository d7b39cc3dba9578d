"""Tangent liveness of a lowered program (pure Python, no GPU): which instructions can see a non-zero tangent.

The dual rules of csrc/sdfk_dualdev.h have two kinds of terms: those that multiply the tangent of the instruction's input
register(s) and those that multiply the tangent of its own parameters. A scene only tests a term that is reached by a
tangent that can be non-zero. This pass propagates "this register may carry a non-zero tangent" through `low.code`, at
register granularity (not per component), and returns per instruction whether its inputs and its parameters are live.

The instruction word is `op | a<<8 | b<<16 | c<<24` with the parameter offset in `code[:, 1]`; kinds and parameter counts
come from aegolius_amd._ops.OPS (C_C: C[a] = f(C[b]); V_C: V[a] = f(C[b]); V_V: V[a] = f(V[b]); V_VV: V[a] = f(V[b], V[c])).
"""
import numpy as np

from aegolius_amd import _ops

# rules whose tangent is zero by design (piecewise-constant maps): their result is dead whatever goes in
ZERO_TANGENT = ("VSIGN", "VHARDBIN", "VEXPFLAG")


class Live:
    """One instruction: its index, opcode name and the two flags."""
    __slots__ = ("index", "name", "input", "param")

    def __init__(self, index, name, input_live, param_live):
        self.index, self.name, self.input, self.param = index, name, bool(input_live), bool(param_live)

    def __repr__(self):
        return "Live(%d, %s, input=%s, param=%s)" % (self.index, self.name, self.input, self.param)


def liveness(low, rows=None, point_mode=False):
    """-> [Live] for every instruction of `low`.

    point_mode: coordinate register 0 (the input point) is live and no parameter is (value_and_grad_points);
    otherwise `rows` are the (channels, n_params) parameter tangents of aegolius_amd.autodiff.parameter_tangents."""
    n_params = int(np.asarray(low.params).size)
    if rows is None:
        moving = np.zeros(n_params, dtype=bool)
    else:
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, n_params)
        moving = np.any(rows != 0.0, axis=0)
    c_live, v_live = set(), set()
    if point_mode:
        c_live.add(0)
    out = []
    for i in range(low.code.shape[0]):
        w, poff = int(low.code[i, 0]), int(low.code[i, 1])
        info = _ops.OPS[w & 255]
        a, b, c = (w >> 8) & 255, (w >> 16) & 255, (w >> 24) & 255
        if info.kind in ("C_C", "V_C"):
            inp = b in c_live
        elif info.kind == "V_V":
            inp = b in v_live
        else:
            inp = b in v_live or c in v_live
        par = bool(np.any(moving[poff:poff + max(info.nparams, 0)]))
        res = (inp or par) and info.name not in ZERO_TANGENT
        regs = c_live if info.kind == "C_C" else v_live
        (regs.add if res else regs.discard)(a)
        out.append(Live(i, info.name, inp, par))
    return out
