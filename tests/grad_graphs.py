"""Graphs of the backward tests (fz_run_block_grad): the supported workloads, two graphs written for the tests, and the refusals."""
import graphs as G
from graphs import DEL, IN, add, fn, lit, mul, sub


def div_sqrt_exp():
    """a feedback with DIV, SQRT and EXP:  ~( 0.5*_1[_1] / (1 + sqrt(_1[_1]*_1[_1] + 0.25)) + 0.3*exp(-0.5*_2) )"""
    y1 = DEL(1, 1)
    den = add(lit(1.0), fn("sqrt", add(mul(y1, y1), lit(0.25))))
    return G.fb(add(("div", mul(lit(0.5), y1), den), mul(fn("exp", mul(lit(-0.5), IN(2))), lit(0.3))))


def rules():
    """two inputs, the data-dependent rules side by side:  max(_1, _2) + min(_1, _2)*0.75 + (|_1| + (_1 > 0.5)*_2) - _2[_1]*_1[_1]"""
    x1, x2 = IN(1), IN(2)
    ff = add(add(fn("max", x1, x2), mul(fn("min", x1, x2), lit(0.75))), add(fn("abs", x1), mul(G.cmp("gt", x1, lit(0.5)), x2)))
    return sub(ff, mul(DEL(2, 1), DEL(1, 1)))


# name -> s-expression builder: every graph the backward must take
SUPPORTED = {
    "integrator": G.integrator,
    "df1": G.df1,
    "df1_cascade6": lambda: G.df1_cascade(6),
    "df1_cascade_params6": lambda: G.df1_cascade_params(6),
    "osc_chain6": lambda: G.osc_chain(6),
    "par4_sum": G.par4_sum,
    "par4_sum_fanout": G.par4_sum_fanout,
    "cross_wire": G.cross_wire,
    "clipped_biquad": G.clipped_biquad,
    "moog_ladder": G.moog_ladder,
    "soft_clip_cascade": G.soft_clip_cascade,
    "envelope_follower": G.envelope_follower,
    "div_sqrt_exp": div_sqrt_exp,
    "rules": rules,
}

# name -> (s-expression builder, compile typed?, a word the refusal's reason holds)
REFUSED = {
    "typed_df1_double": (G.df1_double, True, "typed"),
    "one_pole_readme": (G.one_pole_readme, False, "float64"),
    "complex_gain": (lambda: mul(G.litc(0.6, 0.7), IN(1)), False, "complex"),   # (a complex wire cannot be fed back under fz_compile)
    "modulated_cascade": (lambda: G.df1_cascade_modulated(2), False, "modulator"),
    "lds_ring_comb": (G.lds_ring_comb, False, "LDS"),
    "far_comb": (G.far_comb, False, "HBM"),
}
