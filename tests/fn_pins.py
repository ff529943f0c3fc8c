"""Kernel identities of every graph that existed before the graph functions (abs, sqrt, exp, tanh, min, max) were added.

pins() names, for every zero-argument graph builder of tests/graphs.py and zignal_amd/workloads.py and the BASELINE shapes, the
kernel a launch without a variant runs: kernel_name, kernel_symbol and kernel_code_id (a hash of the generated source, the build
options and the compiler).  tests/golden/graph_pins.json holds the values recorded from the tree before the functions existed;
test_graph_functions_host.py asserts that the library still gives them, i.e. that no existing kernel source or plan changed."""
import inspect

import graphs as G
from zignal_amd import flowz as F
from zignal_amd import workloads as W

SHAPES = [(1 << 20, 4096), (65536, 4096), (4096, 256)]


def builders():
    out = {}
    for mod in (W, G):
        for name, fn in sorted(vars(mod).items()):
            if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != mod.__name__:
                continue
            try:
                if any(p.default is inspect.Parameter.empty for p in inspect.signature(fn).parameters.values()):
                    continue
                e = fn()
            except Exception:  # noqa: BLE001  (helpers that are not graph builders)
                continue
            if isinstance(e, tuple) and e and isinstance(e[0], str):
                out.setdefault(name, e)
    for name, fn in W.BASELINE_GRAPHS.items():
        out["BASELINE:" + name] = fn()
    return out


def _program(e):
    try:
        return F.compile(F.from_sexpr(e))
    except F.FlowzError:
        return F.compile(F.from_sexpr(e), typed=True)


def pins():
    rec = {}
    for name, e in sorted(builders().items()):
        try:
            prog = _program(e)
        except F.FlowzError:
            continue
        for ns, T in SHAPES:
            for tile in (0, prog.recommended_tile_streams()):
                key = f"{name}@{ns}x{T}t{tile}"
                try:
                    rec[key] = [prog.kernel_name(None, ns, T, tile), prog.kernel_symbol(None, ns, T, tile), prog.kernel_code_id(None, ns, T, tile)]
                except F.FlowzError as ex:
                    rec[key] = ["error", str(ex)[:60], ""]
    return rec
