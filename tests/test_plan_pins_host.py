"""The planner's choices pinned: tests/golden/plan_pins.json holds, for a few hundred (graph, variant, shape) cases aimed at the planner's
rules -- partial and flags-only variants, the stream-major bodies and their refusals, tile fitting, the 4 GiB chunk rule, the step back
from two I/O waves, the lockstep step-down, edge stream counts -- the kernel a launch runs (kernel_name, kernel_code_id) or the error it
gets.  Needs no GPU: the kernels are those build() leaves in the kernel cache."""
import json
import os

import fn_pins
from zignal_amd import flowz as F

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plan_pins():
    want = json.load(open(os.path.join(HERE, "golden", "plan_pins.json")))
    builders = fn_pins.builders()
    progs = {}
    got = {}
    for key in want:
        name, v, ns, T, tile = key.split("|")
        if name not in progs:
            progs[name] = fn_pins._program(builders[name])
        var = None if v == "-" else F.make_variant(*map(int, v.split(",")))
        ns, T, tile = int(ns), int(T), int(tile)
        try:
            got[key] = [progs[name].kernel_name(var, ns, T, tile), progs[name].kernel_code_id(var, ns, T, tile)]
        except F.FlowzError as ex:
            got[key] = ["error", str(ex)]
    diff = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not diff, f"{len(diff)} of {len(want)} plans differ, e.g. {sorted(diff.items())[:3]}"
