/* flowz_hip.h -- C ABI of libflowz_hip.so: MI355X (gfx950) evaluator for Flowz flow-graphs.
 *
 * This is the drop-in boundary of the hot path.  The reference has no FFI: its path sits
 * behind a C++ header API (/root/reference/flowz/flowz.hpp).  Each group below names the
 * reference interface it replaces; the C++ front end (include/flowz/flowz.hpp) and the
 * Python mirror (zignal_amd/flowz.py) are thin layers over exactly these entry points.
 *
 * Conventions: plain pointers and sizes, no exceptions cross the boundary.  Functions
 * returning int give FZ_OK (0) or a negative fz_status; fz_last_error() returns a
 * thread-local message for the last failure on the calling thread.
 * All arithmetic is IEEE float32, one rounding per expression node in the user's
 * association order, no FMA contraction, denormals kept (flowz.hpp:769-772,
 * CMakeLists.txt:18).
 */
#ifndef FLOWZ_HIP_H
#define FLOWZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fz_status {
   FZ_OK            =  0,
   FZ_E_INVALID     = -1,   /* bad argument (null, misaligned, size mismatch)              */
   FZ_E_GRAPH       = -2,   /* malformed flow-graph (arity, delay-free loop, ...)          */
   FZ_E_NO_DEVICE   = -3,   /* no HIP device: the product path has no CPU fallback         */
   FZ_E_HIP         = -4,   /* HIP runtime error                                           */
   FZ_E_COMPILE     = -5,   /* hiprtc failed to build the generated kernel                 */
   FZ_E_UNSUPPORTED = -6    /* valid graph, beyond this build (e.g. delay too long)        */
} fz_status;

const char* fz_last_error(void);
const char* fz_version(void);

/* ------------------------------------------------------------------------------------------
 * Expression construction  == the EDSL surface, flowz.hpp:68-93 and :1252-1257.
 * Handles are immutable, reference counted trees; every constructor returns a NEW handle
 * (refcount 1) and retains its operands, so the caller releases what it created
 * (value semantics of proto's copy_domain, flowz.hpp:46-61).  NULL on error.
 * ---------------------------------------------------------------------------------------- */
typedef struct fz_expr fz_expr;

typedef enum fz_op { FZ_OP_ADD = 1, FZ_OP_SUB = 2, FZ_OP_MUL = 3, FZ_OP_DIV = 4, FZ_OP_NEG = 5,
                     /* the comparison and logical operators of C++ (proto::_default applies whatever operator a node is, flowz.hpp:51-55,
                        :769-772): the result is the operator's bool as it behaves in arithmetic -- 1 or 0, taking the type of what it
                        meets next (bool * float is a float multiplication, bool * double a double one); an output frame or a delay
                        line receives it as 1.0f / 0.0f.  Operands are compared in their common type (double if one is), IEEE semantics
                        (every comparison with a NaN is false, != true).  Not for std::complex wires.  a && b, a || b, !a test their
                        operands against zero as C++ does for arithmetic types; both sides are always evaluated (no side effects to skip). */
                     FZ_OP_LT = 6, FZ_OP_LE = 7, FZ_OP_GT = 8, FZ_OP_GE = 9, FZ_OP_EQ = 10, FZ_OP_NE = 11,
                     FZ_OP_NOT = 12, FZ_OP_AND = 13, FZ_OP_OR = 14,
                     /* Graph functions: std::fabs, std::sqrt, std::exp, std::tanh (unary: b is ignored, the operand's input arity is
                        kept, it must have exactly one output wire) and std::min, std::max of <algorithm> (binary).  Each counts as ONE
                        node in fz_info.n_ops.  They work in the wire's C++ type: float, or double when an operand is double (a
                        fz_literal_f64 below it, or a typed FZ_DT_F64 wire); min / max compare and return in the operands' common type.
                          abs(a)    clears the sign bit (exact).
                          sqrt(a)   IEEE correctly rounded; sqrt(-0) = -0, a negative operand gives NaN.
                          min(a, b) (b < a) ? b : a,   max(a, b) (a < b) ? b : a  -- std::min / std::max exactly, signed zeros and the
                                    position of a NaN included: min(NaN, 1) = NaN, min(1, NaN) = 1.
                          exp(a)    within 2 ulp of the correctly rounded result (float: 0.957 ulp at most over all 2^32 inputs;
                                    double: 0.95 ulp at most on 2^22 stratified inputs); exp(+-0) = 1,
                                    exp(-inf) = +0, exp(+inf) = +inf, +inf exactly where the correctly rounded result overflows
                                    (a > 0x1.62e42ep+6 float, a > 0x1.62e42fefa39efp+9 double), gradual underflow.
                          tanh(a)   within 2 ulp (float: 1.437 ulp at most over all 2^32 inputs; double: 1.43 ulp at most on 2^22
                                    stratified inputs); odd bitwise (tanh(-x) = -tanh(x), tanh(+-0) = +-0), |tanh| <= 1, exactly +-1 for
                                    |a| > 10 (float) / 20 (double) and at +-inf, tanh(x) = x for tiny and subnormal x.  Monotone: over all
                                    2^32 float inputs in increasing order the float tanh never steps down, the switch point at 0.55
                                    included (float exp likewise; tools/graph_functions_exhaustive.py).
                        exp and tanh are the library's own algorithm, built from IEEE +, -, *, correctly rounded /, exact scaling by
                        powers of two through the exponent bits and round-to-nearest-even to integer (the 1.5 * 2^(p-1) trick): no FMA,
                        no hardware approximation (v_exp_f32, v_log_f32, a bare v_rcp_f32), no ocml / libm call, no tables.
                          exp:  k = rint(a / ln 2), r = (a - k ln2_hi) - k ln2_lo (k ln2_hi exact), e^r = 1 + (r + r^2 q(r)) with a
                                Chebyshev-fitted q by Horner's rule, then * 2^(k >> 1) (exact) * 2^(k - (k >> 1)) (rounds once).
                          tanh: |a| < 0.55: |a| + |a| (z P(z)), z = a^2; else 1 - 2 / (exp(2 |a|) + 1); the sign of a put back last.
                        A numpy restatement in float32 / float64 arrays gives the kernels' bits for every non-NaN result
                        (tests/fn_ref.py); a NaN result is a NaN, its payload is not specified.
                        std::complex operands: min / max -> FZ_E_GRAPH (C++ has no such operator); abs, sqrt, exp, tanh ->
                        FZ_E_UNSUPPORTED (valid C++, not built here). */
                     FZ_OP_ABS = 15, FZ_OP_SQRT = 16, FZ_OP_EXP = 17, FZ_OP_TANH = 18, FZ_OP_MIN = 19, FZ_OP_MAX = 20,
                     /* std::sin, std::cos, std::log: unary graph functions under the rules above (b is ignored, the operand has exactly one
                        output wire and keeps its input arity, ONE node in n_ops), the library's own algorithms from the same allowed
                        operations: IEEE +, -, *, correctly rounded /, exact exponent-bit scaling, conversions; no FMA, no hardware
                        approximation (v_sin_f32, v_cos_f32, v_log_f32, a bare v_rcp_f32), no ocml / libm call, no tables; branch-free per
                        lane.  tests/fn_ref_trig.py restates them in numpy operation for operation and gives the kernels' bits for every
                        non-NaN result.
                          sin(a), cos(a)  FLOAT32 operands only (a double operand -- a fz_literal_f64 below it or a typed FZ_DT_F64 wire --
                                    is FZ_E_UNSUPPORTED: valid C++, not built here).  The algorithm and constants of the RBJ generator's
                                    sine and cosine: x = (double)a; t = x * 2/pi; k = (int)(t + (t < 0 ? -0.5 : 0.5)) (the conversion
                                    truncates); r = ((x - k h1) - k h2) - k h3 with a three-part pi/2 whose head h1 has 33 bits (k h1
                                    exact); z = r r; s = r + r (z S(z)), c = 1 + z C(z) with the Taylor polynomials (8 and 9 terms) by
                                    Horner's rule; quadrant q = k & 3: sin = s, c, -s, -c and cos = c, -s, -c, s; rounded to float ONCE;
                                    sin returns a itself for a = +-0 (the sum r + r (z S) loses the sign of -0).
                                    The double is within 2^-60 of the true value, so the float is the correctly rounded result except for
                                    arguments within that distance of a rounding boundary: measured below 0.500001 ulp for sin and for cos
                                    over every float with |a| < 2^20 against float64 numpy (tools/graph_functions_exhaustive.py).
                                    DOMAIN: |a| >= 2^20, +-inf and NaN give NaN (beyond that point k h1 is no longer exact; a wider
                                    domain needs a Payne-Hanek reduction).  sin(+-0) = +-0, cos(+-0) = 1; sin is odd bitwise and cos
                                    even bitwise, |sin|, |cos| <= 1, sin(a) = a for tiny and subnormal a (all checked over that domain).
                          log(a)    in the wire's C++ type (float, or double when the operand is double, like exp).  The fdlibm scheme:
                                    a = m 2^e through the exponent bits with m in [sqrt(1/2), sqrt 2) (bits + (bits(1) - bits(sqrt(1/2))),
                                    exponent field - bias = e, mantissa field + bits(sqrt(1/2)) = m; subnormals first scaled by 2^25 /
                                    2^54, exact); f = m - 1, s = f / (2 + f), z = s s, w = z z; R = z (L1 + w (L3 + ..)) + w (L2 + w (L4 + ..))
                                    with L fitted here (Chebyshev fit of (log((1+s)/(1-s))/s - 2)/z on z in [0, 0.0295]: 4 coefficients
                                    float, 7 double); h = (0.5 f) f; t = s (h + R); u = t + e ln2_lo; v = f - (h - u); log = e ln2_hi + v
                                    with exp's two-part ln 2 (e ln2_hi exact).  Within 2 ulp of the correctly rounded result (float:
                                    0.840 ulp at most over all 2^32 inputs; double: 0.826 ulp at most on 2^22 stratified inputs against
                                    mpmath).  log(+-0) = -inf, log(a < 0) = NaN, log(+inf) = +inf, log(1) = +0, NaN gives NaN (payload
                                    unspecified).  Monotone: over all 2^32 float inputs in increasing order the float log never steps
                                    down (tools/graph_functions_exhaustive.py).
                        std::complex operands of sin, cos, log -> FZ_E_UNSUPPORTED (valid C++, not built here), as for abs .. tanh. */
                     FZ_OP_SIN = 21, FZ_OP_COS = 22, FZ_OP_LOG = 23 } fz_op;

fz_expr* fz_placeholder(uint32_t i);                 /* _i          make_placeholder<i>() :78-82   */
fz_expr* fz_delayed(uint32_t i, uint32_t n);         /* _i[_n]      delayed_placeholder   :84-85   */
fz_expr* fz_literal(float value);                    /* terminal held by value  make_terminal :68-72 */
fz_expr* fz_literal_f64(double value);               /* a C++ `double` literal terminal: the operators above
                                                        it evaluate in double (usual arithmetic conversions,
                                                        proto::_default :769-772; test/tests.cpp:200-231),
                                                        delay lines and output frames stay float32 (:1245) */
fz_expr* fz_literal_c32(float re, float im);         /* a std::complex<float> terminal (test/tests.cpp:206-207):
                                                        the wire above it is complex -- two float32 slots
                                                        (re, im) of the output frame; operators follow
                                                        std::complex<float> (scalar mul/div and add touch the
                                                        parts as <complex> does, complex*complex is the
                                                        (ac-bd, ad+bc) of __mulsc3 for finite values; z/w and
                                                        s/w are libgcc's __divsc3 as g++ links it: the four
                                                        parts widened to double, x = (ac+bd)/(cc+dd),
                                                        y = (bc-ad)/(cc+dd), rounded to float once).  Under
                                                        fz_compile a complex wire cannot enter a delay line
                                                        (they are float, :1245; fz_compile_typed stores it)
                                                        nor meet a double operand (no such operator in C++):
                                                        FZ_E_GRAPH                                        */
fz_expr* fz_literal_c64(double re, double im);       /* a std::complex<double> terminal: as fz_literal_c32 with double parts.  Operators
                                                        follow std::complex<double>: z*w is the (ac-bd, ad+bc) of __muldc3, z/w and
                                                        s/w are libgcc's __divdc3 = Smith's method (|c| < |d| ? ratio c/d : ratio d/c;
                                                        both sides are evaluated and selected: FZ_IR_ABSLT / FZ_IR_SELECT); it mixes
                                                        with double scalars only (as in C++: no operator for complex<double> with
                                                        float or complex<float>)                                              */
fz_expr* fz_stream_param(uint32_t k);                /* per-stream, block-constant coefficient k:
                                                        the std::ref terminal of flowz/README.md:42-61,
                                                        one value per stream                          */
fz_expr* fz_uniform(uint32_t k, float initial);      /* uniform run-time coefficient k (same value for
                                                        all streams, constant during a block): what a
                                                        std::ref(x) terminal is when the closure is called
                                                        (flowz/README.md:42-61); set with
                                                        fz_program_set_uniform between blocks             */
fz_expr* fz_modulator(uint32_t k);                   /* the std::ref(x) terminal at SAMPLE rate (flowz/README.md:42-61: the
                                                        reference re-reads the referenced variable on every call, i.e. every
                                                        sample): modulator k has one value per sample of a block, the same
                                                        for all streams, read from the array fz_program_set_modulation names --
                                                        an input wire without the per-stream HBM traffic (scalar loads)       */
fz_expr* fz_arith(fz_op op, fz_expr* a, fz_expr* b); /* any C++ arithmetic, comparison or logical operator,
                                                        _default :769-772, or a graph function; b is ignored
                                                        (may be NULL) for FZ_OP_NEG, FZ_OP_NOT, FZ_OP_ABS,
                                                        FZ_OP_SQRT, FZ_OP_EXP, FZ_OP_TANH, FZ_OP_SIN,
                                                        FZ_OP_COS and FZ_OP_LOG                           */
fz_expr* fz_channel (fz_expr* a, fz_expr* b);        /* a , b       channel_operator   :90           */
fz_expr* fz_parallel(fz_expr* a, fz_expr* b);        /* a | b       parallel_operator  :91           */
fz_expr* fz_sequence(fz_expr* a, fz_expr* b);        /* a |= b      sequence_operator  :92           */
fz_expr* fz_feedback(fz_expr* a);                    /* ~a          feedback_operator  :93           */
void     fz_expr_retain (fz_expr* e);
void     fz_expr_release(fz_expr* e);

/* Static analysis transforms (flowz.hpp:162-246, :443-506; asserted by test/tests.cpp:63-102). */
int fz_input_arity (const fz_expr* e);               /* >= 0, or negative fz_status                   */
int fz_output_arity(const fz_expr* e);
/* per external input wire, deepest delayed read; writes min(n, cap) entries, returns n        */
int fz_max_input_delays(const fz_expr* e, uint32_t* out, uint32_t cap);

/* ------------------------------------------------------------------------------------------
 * compile()  == flowz::compile, flowz.hpp:1233-1249: arity, front panel, feedback
 * resolution, state layout -- at run time instead of C++ template instantiation.
 * Pure host work: succeeds without a GPU.
 * ---------------------------------------------------------------------------------------- */
typedef struct fz_program fz_program;

typedef struct fz_info {
   uint32_t n_in;        /* external input wires  (frame width of `in`)                       */
   uint32_t n_out;       /* output wires          (frame width of `out`)                      */
   uint32_t n_nodes;     /* nodes of the lowered per-sample DAG                               */
   uint32_t n_ops;       /* arithmetic nodes = float32 operations per stream-sample (a graph function node counts as one) */
   uint32_t n_lines;     /* delay lines (one per delayed wire, shared by all its readers)     */
   uint32_t n_state;     /* floats of state per stream = sum of line depths                   */
   uint32_t n_const;     /* distinct uniform float32 coefficients (literal terminals)         */
   uint32_t n_param;     /* per-stream coefficients (highest fz_stream_param index + 1)       */
   uint32_t max_delay;   /* deepest delay line                                                */
   uint32_t n_lds_slots; /* ring-buffer slots kept in LDS (lines deeper than the register cap) */
   uint32_t stage_packable; /* 1 when the graph is a series of isomorphic segments (FZ_VF_STAGE_PACK) */
   uint32_t n_const64;   /* distinct float64 literal terminals                                */
   uint32_t n_out_wires; /* output wires (output_arity); < n_out when some wires are complex         */
   uint32_t n_in_wires;  /* input wires (input_arity); < n_in when a typed program has double / complex inputs */
   uint32_t typed;       /* 1 for fz_compile_typed programs                                           */
   uint32_t n_mod;       /* sample-rate modulators (highest fz_modulator index + 1)                            */
   uint32_t differs_from_reference; /* != 0: the graph holds a feedback ~(a |= b) whose first part keeps that many EXTERNAL inputs for itself
                            while the part behind it reads external inputs too (the graphs of test/tests.cpp:67-77).  The reference's
                            shipped binary_feedback hands that second part the wrong wires (flowz.hpp:1045-1050: tuple_drop<std::min(0, ..)>,
                            "TODO" there); this library routes per the reference's arity table (:162-246) -- e.g.
                            ~(_1 + _2[_1] |= _1[_1] + _2) on (10,1),(20,2),(30,3) gives 1, 3, 16 here and 10, 30, 70 from the shipped header.
                            fz_compile succeeds and leaves a note in fz_last_error()                                          */
} fz_info;

int  fz_compile(const fz_expr* e, fz_program** out);

/* compile() with the wire types of the reference's ResultType transform (flowz.hpp:585-644, asserted by
 * test/tests.cpp:184-232) carried through INPUTS, STATE and OUTPUTS instead of the float state that compile()
 * hard-codes today (flowz.hpp:1245, "TODO" there):
 *   - input wire i arrives as in_dtypes[i] (fz_dtype; NULL or n_in_wires == 0: all float) -- the reference's callable
 *     is a template over its argument types (flowz.hpp:1225-1229), so f(1.0) or f(std::complex<float>{..}) are legal;
 *   - a delay line stores the type that is pushed into it and a delayed read returns that type (tests.cpp:219);
 *     the type of a fed-back wire is what the "absorber" rule of ResultType gives: the least type that is consistent
 *     around the loop, e.g. ~(_1[_1] + 1.0*_2) is double (tests.cpp:224-226); a loop that never meets another type
 *     stays float;
 *   - frames carry every wire in its own type: float = 1 float slot, double = 2 slots (low word, high word: the
 *     frame is a double[] there), std::complex<float> = 2 slots (re, im).  n_in / n_out of fz_info count SLOTS,
 *     n_in_wires / n_out_wires count wires.  FZ_VF_OUT_F64 does not apply (rejected).
 * State rows: double lines come first and take two float rows per delay slot (one row of n_streams doubles);
 * a complex wire has one float line for each part.  Double lines: registers up to 8 samples, LDS rings up to 256.
 * std::complex<double> wires (fz_literal_c64, FZ_DT_CF64 inputs) take four slots: the double of the real part, then
 * the double of the imaginary part; their delay lines are two double lines.                                         */
typedef enum fz_dtype { FZ_DT_F32 = 0, FZ_DT_F64 = 1, FZ_DT_CF32 = 2, FZ_DT_CF64 = 3 } fz_dtype;   /* CF64: 4 slots (re, im doubles) */
int  fz_compile_typed(const fz_expr* e, const uint32_t* in_dtypes, uint32_t n_in_wires, fz_program** out);
/* type of every input wire (fz_dtype); writes min(n, cap), returns n = n_in_wires */
int  fz_program_input_dtypes(const fz_program* p, uint32_t* dtypes, uint32_t cap);
/* storage type of every delay line, in fz_program_lines order: 0 float, 1 double (two state rows per slot),
 * 2 / 3 the real / imaginary part of a std::complex<float> wire (float rows), 4 / 5 the real / imaginary part of a
 * std::complex<double> wire (double lines: two state rows per slot); writes min(n, cap), returns n */
int  fz_program_line_dtypes(const fz_program* p, uint32_t* dtypes, uint32_t cap);
void fz_program_destroy(fz_program* p);
int  fz_program_info(const fz_program* p, fz_info* info);

/* Lowered IR, for inspection and for tests (the product never interprets it on the CPU). */
typedef enum fz_ir_kind {
   FZ_IR_INPUT = 1,   /* a = input wire index                                                  */
   FZ_IR_CONST = 2,   /* a = coefficient slot, value = its float                               */
   FZ_IR_PARAM = 3,   /* a = per-stream coefficient index                                      */
   FZ_IR_DELAY = 4,   /* a = source node, b = n : value of node a, n samples ago               */
   FZ_IR_ADD = 5, FZ_IR_SUB = 6, FZ_IR_MUL = 7, FZ_IR_DIV = 8,   /* a (op) b                    */
   FZ_IR_NEG = 9,     /* -a                                                                    */
   FZ_IR_WIDEN = 10,  /* (double)a : float -> double, exact                                    */
   FZ_IR_NARROW = 11, /* (float)a  : double -> float, one IEEE rounding (both only appear where C++ itself converts
                         inside an operator: the float complex division of libgcc's __divsc3, see fz_arith)           */
   FZ_IR_MOD = 12,    /* a = modulator index: value of sample-rate modulator a at this sample (fz_modulator)          */
   FZ_IR_ABSLT = 13,  /* |a| < |b| ? 1 : 0  (in the operands' type)                                                    */
   FZ_IR_SELECT = 14, /* a != 0 ? b : c   (the data-dependent branch of __divdc3; both sides are evaluated)            */
   FZ_IR_LT = 15, FZ_IR_LE = 16, FZ_IR_GT = 17, FZ_IR_GE = 18, FZ_IR_EQ = 19, FZ_IR_NE = 20,
                      /* a (cmp) b ? 1.0f : 0.0f -- a float32 node (dtype 0) whose operands are compared in double when one of them is     */
   FZ_IR_ABS = 21, FZ_IR_SQRT = 22, FZ_IR_EXP = 23, FZ_IR_TANH = 24,   /* f(a), in a's type (see FZ_OP_ABS ..)                 */
   FZ_IR_MIN = 25, FZ_IR_MAX = 26,    /* std::min / std::max of a and b in their common type; never stage-packed (kinds >= ABSLT) */
   FZ_IR_SIN = 27, FZ_IR_COS = 28,    /* std::sin / std::cos of a, float32 only (see FZ_OP_SIN)                                   */
   FZ_IR_LOG = 29                     /* std::log of a, in a's type; the three are never stage-packed or wave-split either          */
} fz_ir_kind;

typedef struct fz_ir_node {
   uint32_t kind, a, b;
   float value;        /* FZ_IR_CONST, dtype 0 */
   uint32_t dtype;     /* 0 = float32, 1 = float64 (the node's C++ arithmetic type) */
   double value64;     /* FZ_IR_CONST, dtype 1 */
   uint32_t c;         /* third operand (FZ_IR_SELECT) */
} fz_ir_node;

/* nodes are in evaluation (topological) order; writes min(n, cap), returns n */
int fz_program_ir(const fz_program* p, fz_ir_node* nodes, uint32_t cap);
/* node id of each output frame slot (a complex wire takes two: re, im); writes min(n_out, cap), returns n_out */
int fz_program_outputs(const fz_program* p, uint32_t* node_ids, uint32_t cap);
/* arithmetic type of each output frame slot before it is narrowed to the float32 frame: 0 = float, 1 = double,
 * 2 / 3 = real / imaginary part of a std::complex<float> wire; fz_compile_typed programs: 4 / 5 = low / high word
 * of a double wire (never 1: nothing is narrowed), 6 / 7 / 8 / 9 = low / high word of the real, low / high word of
 * the imaginary part of a std::complex<double> wire; fz_compile programs: 10 / 11 = real / imaginary part of a
 * std::complex<double> wire (narrowed to the float frame like code 1)
 * (the ResultType inference of flowz.hpp:585-644 / test/tests.cpp:200-231, with compile()'s float delay
 * lines: a delayed read is float whatever was pushed, flowz.hpp:1245); writes min(n_out, cap), returns n_out */
int fz_program_output_dtypes(const fz_program* p, uint32_t* dtypes, uint32_t cap);
/* delay lines: source node and depth of line l; state rows of line l start at the sum of the
 * depths before it, row (start + j) holds the wire's value at t-1-j (j = 0 newest).
 * Lines deeper than 256 samples are rings in HBM instead: their `depth` rows are ring slots, one
 * extra state row per such line (after all line rows) holds the ring phase p (as a float), and the
 * value at t-1-j sits in slot (p - 1 - j) mod depth.  n_state counts those phase rows.          */
int fz_program_lines(const fz_program* p, uint32_t* src_nodes, uint32_t* depths, uint32_t cap);
/* read / overwrite a uniform coefficient (literal terminal) between blocks */
int fz_program_get_const(const fz_program* p, uint32_t slot, float* value);
int fz_program_set_const(fz_program* p, uint32_t slot, float value);
/* overwrite uniform run-time coefficient k (fz_uniform) between blocks */
int fz_program_set_uniform(fz_program* p, uint32_t k, float value);
/* Sample-rate modulators (fz_modulator): mod_dev is a DEVICE array [n_mod][stride] of floats, stride >= the rows the frame
 * buffers of the following launches hold; sample t of a block (row row0 + t of a window) reads modulator k at
 * mod_dev[k * stride + row0 + t].  The pointer is remembered by the program until it is set again (like fz_program_set_uniform:
 * set it before the launch that needs it; a launch of a graph with modulators and no array fails with FZ_E_INVALID).
 * Graphs with modulators are not stage-packed (their segments run at different times).                                   */
int fz_program_set_modulation(fz_program* p, const float* mod_dev, uint32_t stride);

/* ------------------------------------------------------------------------------------------
 * Kernel variants.  One fused HIP kernel per (graph, variant) is generated and built with
 * hiprtc for gfx950 (building needs no GPU; code objects are cached on disk).
 * ---------------------------------------------------------------------------------------- */
typedef struct fz_variant {
   uint32_t streams_per_lane;  /* 1, 2 (v_pk_* float2) or 4; 0 = choose from n_streams         */
   uint32_t unroll;            /* time steps per prefetch chunk (1..32); 0 = default           */
   uint32_t block_threads;     /* 64..1024, multiple of 64; 0 = default (256)                  */
   uint32_t flags;             /* FZ_VF_* ; 0 = default                                        */
} fz_variant;

enum { FZ_VF_STAGE_PACK = 8u,   /* one stream per lane; the K isomorphic segments of a serial graph (e.g. the
                                   stages of a cascade, after an optional scalar prefix) run skewed in time,
                                   segment j at t-j, and segments i, i+K/2 share one v_pk_* per node; chosen
                                   automatically below 2^18 streams when fz_info.stage_packable          */
       FZ_VF_NO_STAGE_PACK = 16u,
       FZ_VF_PREFETCH3 = 32u,   /* three input chunk buffers: loads run two chunks (2 x unroll steps) ahead
                                   (not with delay lines beyond 256 samples)                              */
       FZ_VF_STREAM_MAJOR = 128u,   /* set by fz_run_block_stream_major (the frame layout is part of the kernel) */
       FZ_VF_SM_LONG = 256u,    /* stream-major frames, 1-in/1-out graphs: the long-run body -- 512-byte runs per stream (unroll 128;
                                   64 selectable), one in-place LDS patch per wave, one wave per SIMD; chosen automatically for
                                   blocks of >= 256 samples; FZ_VF_SM_SHORT keeps the 32-sample chunks.  With streams_per_lane = 2
                                   (unroll 64): the PAIR body -- two streams per lane, every node one packed instruction, halves of
                                   64 samples, 256-byte in-runs and 512-byte out-runs; the default for deep graphs with uniform
                                   coefficients from 2^19 (even) streams on                                              */
       FZ_VF_SM_SHORT = 512u,
       FZ_VF_WAVE_SPLIT = 1024u, /* fewer streams than lanes: a serial graph of K isomorphic segments is cut into W parts of K / W
                                   segments, W waves of a workgroup evaluate the parts for the same 64 streams (the cut wires
                                   travel through LDS, every wave one chunk behind the one before); one stream per lane,
                                   block_threads counts the streams of a workgroup (a multiple of 64).  This bit: W = 2;
                                   FZ_VF_WAVES(3), FZ_VF_WAVES(4): three / four parts.  Chosen automatically for few streams */
       FZ_VF_WAVE_SPLIT3 = 2048u,
       FZ_VF_IO_WAVE = 32768u,  /* one more wave per 64 streams does all the frame I/O: it loads the input rows two rounds ahead and
                                   hands them to the compute wave(s) through LDS, and stores the rows they hand back; the compute
                                   wave is left with arithmetic and LDS accesses.  Alone (a stage-packable graph: one compute wave
                                   + one I/O wave, 4 such pairs per workgroup) or together with FZ_VF_WAVES(n)                   */
       FZ_VF_LOCKSTEP = 524288u, /* time-major / tiled frames: the waves of a workgroup meet at a barrier after every chunk and so walk the
                                   same rows at the same time -- with plain time-major frames of many streams (rows megabytes apart)
                                   that keeps the pages a CU has in flight few; chosen automatically there                        */
       FZ_VF_GRID_SYNC = 8388608u, /* with FZ_VF_LOCKSTEP: the workgroups of one XCD (one contiguous 1/8 of every row) also walk the rows together:
                                   arrival counters in device memory (zeroed in stream order before the launch), bounded waits -- never a
                                   hang, never a different bit; chosen automatically when the chip holds all workgroups at once      */
       FZ_VF_IO_WAVE2 = 33554432u, /* with FZ_VF_IO_WAVE: TWO I/O waves per tuple -- one loads the input rows, one stores the output rows (chosen automatically for
                                   stage-packable graphs of <= 64 operations between 32 768 and 65 536 streams: one compute wave per SIMD next to them).  A wave
                                   issues its vector-memory instructions in order, one row of 64 streams x 4 bytes each: at one I/O wave per
                                   tuple that wave's 2 x n_samples instructions are what a round waits for (profiles/r04/few_streams_floor.txt) */
       FZ_VF_OUT_F64 = 64u };   /* `out` holds float64 frames [..][n_out] of doubles (pass the double* cast to
                                   float*): the results of graphs with double literals leave un-narrowed, float
                                   wires are widened exactly (tuple<double> results, test/tests.cpp:201-231)   */
/* bits 10..11 of flags: wave split into n = 2, 3 or 4 parts (see FZ_VF_WAVE_SPLIT) */
#define FZ_VF_WAVES(n) ((n) >= 2 && (n) <= 4 ? ((uint32_t)((n) - 1) << 10) : 0u)
/* bits 20..22 of flags: at most n workgroups per CU (the kernel pads its LDS); 0 = as many as fit.
 * Fewer, fatter waves keep fewer frame tiles in flight: which occupancy streams fastest from HBM depends
 * on the board -- let fz_program_tune measure it                                                   */
#define FZ_VF_MAX_WG(n) (((uint32_t)(n) & 7u) << 20)
/* bits 0..2, 12..14, 16..18 and 27 are reserved (FZ_E_INVALID): rounds 1-5 had experiment knobs there (cache policies, the SLP vectoriser, the
 * plain block order); those are compile-time switches of the kernel source now (FLOWZ_HIP_EXTRA_OPTS).  The library
 * names kernels of its own with some of them (the adjoint kernels, the PCM kernel): no caller's variant can */

int fz_program_build(fz_program* p, const fz_variant* v);           /* JIT (or cache hit) only   */
/* the same with the variant's automatic fields resolved as a launch of this block shape would: the shape of a launch is
 * (n_streams, n_samples, tile_streams) -- tile_streams as for fz_run_block_tiled, 0 = plain time-major rows (the library's choice
 * depends on the layout: see FZ_VF_LOCKSTEP); stream-major frames are named by FZ_VF_STREAM_MAJOR in v->flags            */
int fz_program_build_for(fz_program* p, const fz_variant* v, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams);
/* Part k of the wave split into n_parts (FZ_VF_WAVES(n_parts); n_parts = 1: the graph itself next to an I/O wave) as a
 * program of its own, for inspection (fz_program_ir, fz_program_lines, fz_program_info): input = the cut wire before the
 * part (the graph input for k = 0), output = the cut wire behind it; constant slots are the parent's.  FZ_E_UNSUPPORTED when
 * the graph does not split that way.  Destroy with fz_program_destroy.                                                */
int fz_program_wave_part(const fz_program* p, uint32_t n_parts, uint32_t k, fz_program** out);
/* Registers, LDS and scratch memory of a variant's kernel, from the code object's metadata (JITs it; no device needed).
 * The unroll of a variant is an UPPER bound for time-major / tiled frames: a kernel whose prefetch buffers and delay lines
 * do not fit the register file would keep some of them in scratch memory, so fz_run_block halves the unroll until nothing
 * spills (stream-major frames keep theirs: it is also the length of a stream's run in memory).  as_launched = 1: the kernel that
 * fz_run_block launches (`unroll` = what is left of the variant's); 0: the variant exactly as given.                   */
typedef struct fz_kernel_resources {
   uint32_t vgprs, agprs, sgprs;
   uint32_t scratch_bytes;      /* per lane; 0 = nothing spills */
   uint32_t lds_bytes;          /* static LDS of a workgroup */
   uint32_t vgpr_spills, sgpr_spills;
   uint32_t unroll;
} fz_kernel_resources;
int fz_program_kernel_resources(fz_program* p, const fz_variant* v, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams,
                                int as_launched, fz_kernel_resources* out);
/* name of the variant's kernel, e.g. "fz_block_kernel_p2u16b256f2097152" (streams per lane, rows per chunk, lanes per workgroup,
 * flags): exactly the kernel a launch of the shape (n_streams, n_samples, tile_streams) runs -- one resolution shared with the
 * launch path; returns length.  (A plain time-major block whose laps leave a few streams over runs a SECOND kernel next to them, on those
 * streams: name, symbol, code id and resources describe the laps' kernel; fz_program_build_for builds both.) */
long fz_program_kernel_name(fz_program* p, const fz_variant* v, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams,
                            char* buf, size_t cap);
/* ... and the SYMBOL of that kernel as profilers show it (rocprofv3 --kernel-trace --stats): the name + "_g<8 hex digits>", a tag of
 * the graph's structure -- two graphs that run the same variant are different rows of a profile (graphs that differ only in
 * coefficient values share the symbol and the code object) */
long fz_program_kernel_symbol(fz_program* p, const fz_variant* v, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams,
                              char* buf, size_t cap);
/* ... and the identity of that kernel's CODE: 16 hex digits, a hash of (generated source, build options, compiler identity) -- the file name of
 * its code object in the kernel cache.  The symbol names variant and graph; this names the instructions: counters measured on one build
 * of a kernel are not this run's when the id differs (profiles/pmc_traffic.json is keyed by it). */
long fz_program_kernel_code_id(fz_program* p, const fz_variant* v, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams,
                               char* buf, size_t cap);
/* An expression as text (one line per node of the DAG, values as bit patterns) and back: what a kernel manifest records of a program.
 * fz_expr_recipe returns the length and writes <= cap bytes; fz_expr_from_recipe returns a new reference, NULL (+ fz_last_error) for
 * text that is not a recipe. */
long fz_expr_recipe(const fz_expr* e, char* buf, size_t cap);
fz_expr* fz_expr_from_recipe(const char* text);
/* Kernel manifests.  With FLOWZ_HIP_MANIFEST=<file> in the environment every kernel a process resolves for the first time is appended to
 * <file> as (the program's expression, input types, variant).  fz_manifest_build replays such a file: compiles the programs again and
 * builds -- in n_workers parallel compiler processes, no GPU needed -- whatever the kernel cache does not hold yet.  The records name
 * expressions and variants, not generated code: a replay after the library changed builds the new kernels of the same launches.
 * counts[4] = {records, already in the cache, built now, failed (a graph or variant this build no longer accepts)}. */
int fz_manifest_build(const char* path, uint32_t n_workers, uint32_t* counts);
/* generated HIP source of a variant (skeleton + graph body); returns length, writes <= cap    */
long fz_program_source(fz_program* p, const fz_variant* v, char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------
 * fz_run_block -- the hot path: stateful_lambda::operator() (flowz.hpp:1225-1229) applied to
 * n_samples consecutive samples of n_streams independent closures in ONE kernel launch
 * (the caller's per-sample loop, test/benchmark.cpp:137-147, moves into the kernel).
 *
 * All pointers are DEVICE pointers, 16-byte aligned, owned by the caller:
 *   in     [n_samples][n_streams][n_in]   time-major interleaved frames (NULL iff n_in == 0)
 *   out    [n_samples][n_streams][n_out]
 *   state  [n_state][n_streams]  in/out; zero it before the first block (flowz.hpp:1245);
 *          carries the closure state from block to block (may be NULL iff n_state == 0)
 *   params [n_param][n_streams]  (NULL iff n_param == 0)
 * n_samples == 0 or n_streams == 0 is an empty block: FZ_OK, nothing is touched.
 * Asynchronous on `hip_stream` (hipStream_t, NULL = default stream); the caller synchronises.
 * `v` may be NULL (all defaults).  A program may run concurrently on different state buffers.
 *
 * WHICH KERNEL RUNS (v == NULL): the plan fz_program_tune measured for this (n_streams, tile_streams, device) -- in this process or,
 * persisted, in an earlier one --, else the library's static choice.  A launch never measures anything by itself.
 * Opt-in, FLOWZ_HIP_AUTOTUNE=1 in the environment (rounds 3-5 did this by default): the first big launch of a shape (the block is the
 * whole buffer, n_streams * n_samples >= 2^26) makes fz_program_tune's measurement on the caller's buffers before it runs:
 *   - it synchronises `hip_stream` and takes the time of a few dozen blocks (>= 100 ms of warm-up, every candidate timed twice);
 *     a candidate replaces the library's static choice only when it wins by more than 3 % (fz_program_tune: 1.5 %);
 *   - it allocates a copy of `state` (n_state * n_streams floats), runs the candidates on the caller's in / out / state buffers and
 *     puts the state back; a state that cannot be put back is FZ_E_HIP (the message says so), never a silent advance; without room
 *     for the copy nothing is measured;
 *   - only candidates whose code objects are already built (in memory or in the kernel cache) take part, nothing is compiled for
 *     it; a candidate that fails -- a HIP error included -- is skipped, and if the measurement itself fails the library's static
 *     choice runs: the launch fails only where a plain launch would;
 *   - it is skipped while `hip_stream` is being captured into a hipGraph, when `in` and `out` overlap, and for windows;
 *   - other launches of the same shape on this program wait until the plan is known (they then use it).
 * ---------------------------------------------------------------------------------------- */
int fz_run_block(fz_program* p, const float* in, float* out, float* state, const float* params,
                 uint64_t n_streams, uint32_t n_samples, const fz_variant* v, void* hip_stream);

/* Same hot path with STREAM-TILED frames, the layout recommended for HBM3E on MI355X:
 *   in   [n_streams / tile_streams][n_samples][tile_streams][n_in]
 *   out  [n_streams / tile_streams][n_samples][tile_streams][n_out]
 * i.e. every tile of tile_streams adjacent streams is its own time-major block.  32 KiB row
 * segments (tile_streams * n_in * 4 bytes; 8192 streams for one wire) measured +15...20 % over
 * 4 MiB rows (profiles/r01/hbm_copy_patterns_microbench.txt).  n_streams must be a multiple of
 * tile_streams and tile_streams a multiple of streams_per_lane * block_threads;
 * tile_streams == 0 or == n_streams is fz_run_block.  state / params stay [rows][n_streams]. */
int fz_run_block_tiled(fz_program* p, const float* in, float* out, float* state, const float* params,
                       uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams,
                       const fz_variant* v, void* hip_stream);

/* tile_streams that makes the row segments ~32 KiB for this graph's frame widths (power of two) */
/* A block that is a WINDOW in time of larger frame buffers: samples [row0, row0 + n_samples) of buffers
 * holding rows_total samples (per tile when tile_streams != 0, else time-major).  Lets a long stream-tiled
 * recording be processed in pieces -- e.g. one block per control period with new coefficients -- without
 * re-laying it out.                                                                                     */
int  fz_run_block_window(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
                         uint32_t rows_total, uint32_t row0, uint32_t n_samples, uint32_t tile_streams, const fz_variant* v,
                         void* hip_stream);
/* The block kernel on STREAM-MAJOR buffers, without a layout pass: in [n_streams][rows_total][n_in],
 * out [n_streams][rows_total][n_out] -- one contiguous buffer per stream, as every closure of the reference
 * consumes its samples (test/benchmark.cpp:137-147); the block is the window [row0, row0 + n_samples).
 * Waves fetch [64 streams][unroll samples] patches along the rows and transpose them through LDS.  One
 * stream per lane (no lane or stage packing: VALU-bound for deep graphs at large stream counts), no delay
 * lines beyond 256 samples, float32 frames; rows_total * n_in, row0 * n_in (and the same for n_out) must
 * be multiples of 4 floats.  For the fastest path convert once with fz_transpose_frames instead.  A graph
 * with a delay line beyond 256 samples runs on these buffers through fz_run_block_far_stream_major.      */
int  fz_run_block_stream_major(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
                               uint32_t rows_total, uint32_t row0, uint32_t n_samples, const fz_variant* v, void* hip_stream);
uint32_t fz_recommended_tile_streams(const fz_program* p);

/* Plan selection (what FFTW_MEASURE is to FFTW): time the candidate kernel variants of this program
 * for this shape on the caller's own device buffers and remember the fastest; later fz_run_block /
 * fz_run_block_tiled / fz_bank_process* calls with the same (n_streams, tile_streams) on this device and
 * variant == NULL use it.  All variants compute bit-identical results.  The buffers are used as by
 * fz_run_block_tiled (tile_streams 0: time-major) for a few dozen blocks: `out` is overwritten and
 * `state` advances -- reset it afterwards.  chosen / chosen_ms (may be NULL): the winner and its time
 * per block.  Synchronises hip_stream.  (The boards are power-managed -- a kernel at the package power
 * cap runs its first ~100 ms faster than it sustains --, so the default is run for >= 100 ms first and
 * every candidate is then timed twice, in a forward and a backward pass over the list.)            */
int fz_program_tune(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
                    uint32_t n_samples, uint32_t tile_streams, void* hip_stream, fz_variant* chosen, float* chosen_ms);

/* The winner is also PERSISTED: a line in <kernel cache dir>/plans.txt keyed by (graph structure -- coefficient values do
 * not matter --, n_streams, tile_streams, the board's UUID); the first launch of that shape without a variant in a later
 * process picks it up, so callers that tuned once never sit on the library default again.  FLOWZ_HIP_NO_PLAN_CACHE=1
 * disables reading and writing.  fz_program_plan: the variant such a launch would use now on the current device
 * ({0,0,0,0} = library default).                                                                                  */
int fz_program_plan(fz_program* p, uint64_t n_streams, uint32_t tile_streams, fz_variant* out);

/* the variants fz_program_tune would measure for this shape (the first entry is the library default {0,0,0,0});
 * writes min(n, cap) entries, returns n.  Pure host work: lets a build step pre-compile them (fz_program_build). */
int fz_program_tune_candidates(fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams, fz_variant* out, uint32_t cap);

/* ------------------------------------------------------------------------------------------
 * fz_run_block_grad -- the backward of ONE block (reverse mode).  The forward block maps
 * (x[0..T), s0, p, c) to (y[0..T), s_T): x the input frames, s0 the state before the block, p the
 * per-stream coefficients (fz_stream_param), c the uniform coefficient slots (literals and
 * fz_uniform: fz_info.n_const).  Given ybar = dL/dy and (optionally) sbar_T = dL/ds_T it computes
 * xbar, sbar0, pbar and cbar, where cbar is PER STREAM ([n_const][n_streams]: no reduction over the
 * streams).  The result is the reverse-mode derivative of exactly the float32 computation of the
 * forward kernels: the lowered IR (fz_program_ir) in evaluation order.
 *
 * Rules per node (g its adjoint, v its forward value, a / b its operands):
 *   ADD  abar += g, bbar += g          SUB  abar += g, bbar -= g          NEG  abar -= g
 *   MUL  abar += g*b, bbar += g*a      DIV  q = g/b; abar += q, bbar -= q*v
 *   SQRT abar += g*(0.5/v)             EXP  abar += g*v                   TANH abar += g*(1 - v*v)
 *   SIN  abar += g*cos(a)              COS  abar -= g*sin(a)              LOG  abar += g/a   -- cos(a) / sin(a): the library's own
 *        functions (FZ_OP_COS / FZ_OP_SIN) on the operand's forward value; each contribution is formed, then added
 *   ABS  abar += g if a > 0, abar -= g if a < 0, nothing otherwise (a = +-0 or NaN)
 *   MIN  (b < a) ? bbar += g : abar += g      MAX  (a < b) ? bbar += g : abar += g   -- all of g to the operand std::min /
 *        std::max returned (their NaN and signed-zero rules decide which)
 *   LT .. NE (and !, &&, || after lowering): derivative zero, NO arithmetic -- an infinite or NaN adjoint never leaks through a
 *        comparison; a node that only feeds comparisons has no adjoint and contributes nothing either.
 *   CONST slot k: cbar[k] += g (equal literal bit patterns share a slot: its cbar sums all uses -- the derivative with respect to
 *        the slot's value, which fz_program_set_const changes for every use at once); PARAM k: pbar[k] += g; INPUT wire w: xbar[w] = g
 *        (the sum of the wire's input nodes in node order; +0 for a wire no adjoint reaches).
 * Delay lines: the adjoint state has exactly the layout of the state (fz_program_lines): row start + j holds the adjoint of the
 * wire's value at t-1-j.  sbar_T comes in that layout and sbar0 goes out in it, so blocks chain backwards: sbar0 of block k is the
 * sbar_T of block k-1 (the same buffer may be passed as both).
 *
 * ORDER OF OPERATIONS (float32, one rounding per operation, no FMA).  Rows t = T-1 down to 0.  At row t every node's adjoint starts
 * as -0.0f (the identity of IEEE addition: the first contribution IS the adjoint, bit for bit) and receives, in this order:
 *   1. the ybar of every output slot that names the node, in slot order;
 *   2. the pending line adjoint: for the line whose source the node is, row `start` of the adjoint state after row t;
 *      then that line's rows move one up (row start + j - 1 := row start + j) and its deepest row becomes -0.0f;
 *   3. the contributions of its consumers, in DECREASING node order (a consumer gives to operand a, then to operand b;
 *      a contribution is formed -- e.g. g*b -- before it is added).
 * Then, in the same decreasing walk, the node's finished adjoint g goes on: a DELAY node adds g into the adjoint state row it
 * reads, a PARAM / CONST node adds g into its pbar / cbar accumulator (one addition per row and node: the step's adjoint is
 * formed before it is added).  The accumulators run over the rows T-1 .. 0 starting from what the caller passed in, so the bits
 * depend on the inputs only -- not on launch geometry, checkpoint stride or stream count, and no atomics are used -- and
 * the backward of block 2 followed by the backward of block 1 on the same accumulators gives the bits of one block of 2T.
 * tests/adjoint_ref.py restates this order in numpy.
 *
 * Scope: fz_compile programs whose lowered graph is float32 throughout (no float64 literal, no complex wire), whose delay lines
 * all live in registers (max_delay <= 8: no LDS or HBM ring) and which read no modulator; node kinds INPUT, CONST, PARAM, DELAY,
 * ADD, SUB, MUL, DIV, NEG, LT .. NE, ABS, SQRT, EXP, TANH, MIN, MAX, SIN, COS, LOG.  Anything else: FZ_E_UNSUPPORTED, fz_last_error() names why.
 * Two frame layouts, one entry point each: fz_run_block_grad takes time-major frames, in / out_grad / in_grad as
 * [T][n_streams][wire]; fz_run_block_grad_stream_major takes stream-major buffers [n_streams][rows_total][wire] -- the layout of
 * fz_run_block_stream_major, and of a [batch, time] tensor -- and differentiates the window of rows [row0, row0 + n_samples).
 * Stream-tiled frames are not taken.  The order of operations above holds for both: the layout moves the frames, it does not
 * change a bit of any result.  State, parameters, the accumulators and the workspace are [row][n_streams] in both.
 *
 * Pointers as for fz_run_block: device pointers, 16-byte aligned, asynchronous on hip_stream (hipStream_t, NULL = default).
 * Output buffers must not overlap the inputs, the workspace or each other, except state0_grad == state_grad.  The uniform
 * coefficients are the program's current constants, as for a forward launch.  n_streams == 0 or n_samples == 0: FZ_OK, nothing
 * is touched.
 *
 * fz_run_block_grad_stream_major: the same fz_grad_args; in / out_grad / in_grad are buffers of rows_total rows per stream (their
 * extents, n_streams * rows_total * wires floats, are what the overlap rule looks at), the workspace is what
 * fz_program_grad_workspace answers for (n_streams, n_samples, checkpoint_rows).  row0 + n_samples <= rows_total; rows_total * n_in,
 * row0 * n_in, rows_total * n_out and row0 * n_out are multiples of 4 floats (the rule of fz_run_block_stream_major; n_samples is
 * free): FZ_E_INVALID otherwise.  Rows of in_grad outside the window are not written, so consecutive windows fill one buffer; they
 * chain through state0_grad and the accumulators like consecutive blocks.
 * ---------------------------------------------------------------------------------------- */
typedef struct fz_grad_args {
   uint32_t struct_size;         /* sizeof(fz_grad_args); a smaller or unknown size is FZ_E_INVALID        */
   uint32_t checkpoint_rows;     /* 0 = library default; else a power of two <= 32: the stride of the saved states */
   const float* in;              /* [T][n_streams][n_in]    forward input of the block (NULL iff n_in == 0) */
   const float* state;           /* [n_state][n_streams]    state BEFORE the block (read only)              */
   const float* params;          /* [n_param][n_streams]                                                    */
   const float* out_grad;        /* [T][n_streams][n_out]                                                   */
   const float* state_grad;      /* [n_state][n_streams]    dL/d(state after the block); NULL = zero        */
   float* in_grad;               /* [T][n_streams][n_in]    written;  NULL = not computed                   */
   float* state0_grad;           /* [n_state][n_streams]    written;  NULL = not computed; may == state_grad */
   float* param_grad;            /* [n_param][n_streams]    ADDED TO; NULL = not computed                   */
   float* const_grad;            /* [n_const][n_streams]    ADDED TO; NULL = not computed                   */
   void*  workspace; uint64_t workspace_bytes;   /* device scratch of at least fz_program_grad_workspace bytes */
} fz_grad_args;
/* FZ_OK, or FZ_E_UNSUPPORTED with the reason in fz_last_error(); host only */
int fz_program_grad_check(const fz_program* p);
/* workspace bytes of a backward of this shape: ceil(n_samples / C) * n_state * n_streams * 4, C the checkpoint stride
 * (checkpoint_rows, or the library default for 0) -- the state before every C-th row */
int fz_program_grad_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t checkpoint_rows, uint64_t* bytes);
/* registers and scratch of the adjoint kernel (JITs it, no device needed); `unroll` = the checkpoint stride it uses */
int fz_program_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out);
/* its symbol, fz_adjoint_kernel_c<C>b<lanes per workgroup>_g<graph tag>; returns the length, writes <= cap bytes */
long fz_program_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
int fz_run_block_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream);
int fz_run_block_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                   uint32_t n_samples, void* hip_stream);
/* The same inspection per frame layout.  FZ_GRAD_TIME_MAJOR answers what the two functions above answer.  FZ_GRAD_STREAM_MAJOR is
 * the kernel of fz_run_block_grad_stream_major: its symbol is fz_adjoint_sm_kernel_c<C>r<R>b<lanes per workgroup>_g<graph tag>, R the
 * rows of the LDS patch its frames move through (a multiple of C and of 4); lds_bytes is the patches of one workgroup.
 * fz_program_grad_source_for: the kernel's whole source (generated configuration and body, hand-written skeleton), as
 * fz_program_source gives it for a forward kernel. */
enum { FZ_GRAD_TIME_MAJOR = 0, FZ_GRAD_STREAM_MAJOR = 1 };
int fz_program_grad_resources_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, fz_kernel_resources* out);
long fz_program_grad_kernel_symbol_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
long fz_program_grad_source_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);

/* fz_run_block_ring_grad -- fz_run_block_grad for graphs with delay lines DEEPER THAN 8 SAMPLES (combs, echoes, plucked strings): a
 * call family of its own, time-major frames, the plain backward (dL/dy given).  fz_grad_args is taken unchanged: fields, nullability,
 * the accumulators that are added to, state0_grad == state_grad and every argument check mean what they mean for fz_run_block_grad,
 * and every check runs before a device is needed.
 *
 * THE CONTRACT: the bits are those of the ORDER OF OPERATIONS of fz_run_block_grad, rules 1 - 4 as they stand, for a line of any
 * depth (the adjoint state of a line of depth D has D rows; rule 2 moves them one up whatever D is).  They depend on the inputs
 * alone -- not on the checkpoint stride, the lanes per workgroup or the stream count; no atomics, no FMA -- and the backward of
 * block 2 followed by the backward of block 1 on the same accumulators (state0_grad of block 2 as state_grad of block 1) gives the
 * bits of one block of 2T, also where a block is shorter than a line is deep.  tests/adjoint_ref.py restates the order for any depth.
 *
 * Scope: what fz_program_grad_check accepts, and graphs whose only objection there is float delay lines of depth 9 .. 256 (the lines
 * the forward kernels keep as rings in LDS).  For a graph without such a line these calls ARE the fz_..._grad_ calls: the same
 * kernel, symbol, workspace and bits.  Still refused, with the reasons of fz_program_grad_check: lines deeper than 256 samples (rings
 * in HBM), typed programs, float64 nodes, complex wires, modulators.  Refused here alone: graphs whose deep lines hold more samples
 * than the LDS of a workgroup has room for at 64 lanes (4 bytes per sample and lane, 163 840 bytes: 640 samples) -- the reason names
 * the bytes.  fz_run_block_grad, its stream-major twin and the plain recording calls keep refusing such graphs: stream-major buffers
 * are fz_run_block_ring_grad_stream_major, whole recordings fz_run_recording_ring_grad[_stream_major].  The fused loss is
 * fz_run_block_ring_loss_grad, below fz_run_block_loss_grad.
 *
 * The kernel, fz_adjoint_ring_kernel_c<C>b<lanes per workgroup>_g<graph tag>: lines of depth <= 8 are kept as fz_run_block_grad keeps
 * them (rows in registers, a checkpoint every C rows).  Of a deep line the forward sweep writes the source's value of every row into a
 * tape in the workspace, which the backward sweep reads the delayed values from; the line's pending adjoints live in an LDS ring of D
 * slots per lane.  Lanes per workgroup: the largest of 256 / 128 / 64 whose rings leave room for two workgroups in a compute unit's
 * LDS, failing that the largest that fits one.  C: checkpoint_rows, or for 0 the library default -- 16, halved while
 * C * (n_register_state + n_in + n_ring_reads) exceeds 64 (n_register_state: the state rows of the lines of depth <= 8, n_ring_reads:
 * the distinct (deep line, delay) pairs the graph reads).
 * Workspace: (ceil(n_samples / C) * n_register_state + n_samples * n_ring_lines) * n_streams * 4 bytes; fz_program_ring_grad_workspace
 * answers it (for a graph without a deep line: what fz_program_grad_workspace answers). */
int fz_program_ring_grad_check(const fz_program* p);
int fz_program_ring_grad_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t checkpoint_rows, uint64_t* bytes);
/* registers, scratch and LDS bytes of the kernel (JITs it, no device needed); `unroll` = the checkpoint stride it uses */
int fz_program_ring_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out);
long fz_program_ring_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
long fz_program_ring_grad_source(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
int fz_run_block_ring_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream);

/* fz_run_block_loss_grad -- the backward of one block where dL/dy is not given but FORMED IN THE KERNEL from a target, under a
 * squared-error loss.  The adjoint kernel re-evaluates every step of the block anyway: it holds y when it needs dL/dy, so neither y
 * nor dL/dy has to cross HBM.
 *
 * THE RULE (stated here once).  With y the float32 output of the forward step (the bits of fz_run_block) and k = grad_scale:
 * rows t = T-1 down to 0; within a row the output slots j in ascending order:
 *      e       = y[j] - target[t][j]        one rounding
 *      ybar[j] = e * k                      one rounding
 *      loss    = loss + e * e               the product rounded, then the sum; ONE accumulator per stream
 * The accumulator starts from what the caller's loss[stream] holds: `loss` is ADDED TO, like param_grad, so blocks chain bitwise
 * (the backward of block 2, then of block 1 on the same buffer, gives the bits of one block of 2T).  loss == NULL: not computed.
 * ybar then enters rule 1 of the ORDER OF OPERATIONS above unchanged, and everything after it is fz_run_block_grad's text word for
 * word: every gradient bit equals fz_run_block_grad given that ybar, the bits depend on the inputs only, no atomics, no FMA.
 * The kernel knows no reduction: for the mean over everything pass k = 2 / (T * n_streams * n_out) and multiply the sum of the
 * per-stream losses by 1 / (T * n_streams * n_out).
 *
 * fz_loss_grad_args is fz_grad_args with `target` (the layout of out) where out_grad was, grad_scale, `loss` and `out`: if out is not
 * NULL, y is written there from the second sweep, with the bits of fz_run_block -- the only write the plain backward does not make.
 * state_grad is accepted as before, so a caller can still walk blocks backwards.
 * Scope: fz_program_grad_check's.  Workspace: fz_program_grad_workspace's.  Checks, before a device is needed, each naming its reason:
 * the scope refusals of the backward; n_out == 0: FZ_E_INVALID (nothing to compare); then an empty block (n_streams == 0 or
 * n_samples == 0): FZ_OK, nothing touched; target == NULL: FZ_E_INVALID; pointer alignment, overlap and the 2^30-streams rule as for
 * fz_run_block_grad, with loss and out counted as outputs (they overlap nothing, target included).
 * fz_run_block_loss_grad takes time-major frames; fz_run_block_loss_grad_stream_major stream-major buffers, windows and alignment
 * exactly as fz_run_block_grad_stream_major: rows of in_grad and of out outside the window are never written.  The layout does not
 * change a bit.  The inspection calls take (checkpoint_rows, layout) like their _grad_ twins; the kernels have symbols of their
 * own, fz_adjoint_loss_kernel_c<C>b<lanes>_g<tag> and fz_adjoint_loss_sm_kernel_c<C>r<R>b<lanes>_g<tag>, with the C, the R and the LDS
 * bytes of the plain adjoint kernels (the target travels in the patch part that carries dL/dy there, and y leaves through it). */
typedef struct fz_loss_grad_args {
   uint32_t struct_size;         /* sizeof(fz_loss_grad_args); a smaller or unknown size is FZ_E_INVALID   */
   uint32_t checkpoint_rows;     /* as fz_grad_args                                                         */
   const float* in;              /* [T][n_streams][n_in]    forward input of the block (NULL iff n_in == 0) */
   const float* state;           /* [n_state][n_streams]    state BEFORE the block (read only)              */
   const float* params;          /* [n_param][n_streams]                                                    */
   const float* target;          /* [T][n_streams][n_out]   what y is compared with                         */
   const float* state_grad;      /* [n_state][n_streams]    dL/d(state after the block); NULL = zero        */
   float* in_grad;               /* [T][n_streams][n_in]    written;  NULL = not computed                   */
   float* state0_grad;           /* [n_state][n_streams]    written;  NULL = not computed; may == state_grad */
   float* param_grad;            /* [n_param][n_streams]    ADDED TO; NULL = not computed                   */
   float* const_grad;            /* [n_const][n_streams]    ADDED TO; NULL = not computed                   */
   float* loss;                  /* [n_streams]             sum of e * e, ADDED TO; NULL = not computed     */
   float* out;                   /* [T][n_streams][n_out]   y, written; NULL = not written                  */
   void*  workspace; uint64_t workspace_bytes;   /* device scratch of at least fz_program_grad_workspace bytes */
   float  grad_scale;            /* k of the rule                                                           */
} fz_loss_grad_args;
int fz_run_block_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream);
int fz_run_block_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                        uint32_t n_samples, void* hip_stream);
int fz_program_loss_grad_resources_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, fz_kernel_resources* out);
long fz_program_loss_grad_kernel_symbol_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
long fz_program_loss_grad_source_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);

/* fz_run_block_ring_loss_grad -- fz_run_block_loss_grad for graphs with delay lines DEEPER THAN 8 SAMPLES: the member of the
 * fz_run_block_ring_grad family that forms dL/dy in the kernel.  fz_loss_grad_args is taken unchanged; time-major frames only.
 *
 * THE CONTRACT needs no rule of its own.  THE RULE of fz_run_block_loss_grad applies as written there (e, ybar = e * k, loss += e * e;
 * rows T-1 down to 0, output slots ascending, one rounding per operation, one accumulator per stream that is ADDED TO); ybar then
 * enters rules 1 - 4 of the ORDER OF OPERATIONS as fz_run_block_ring_grad states them for a line of any depth.  Hence every gradient
 * bit equals fz_run_block_ring_grad given that ybar, `out` has the bits of fz_run_block, the bits do not depend on the checkpoint
 * stride, the lanes per workgroup or the stream count, and two blocks chain bitwise through state0_grad, param_grad, const_grad and
 * loss, also where a block is shorter than a line is deep.
 *
 * Scope: fz_program_ring_grad_check's.  Checkpoint stride, lanes per workgroup and workspace: those of fz_run_block_ring_grad
 * (fz_program_ring_grad_workspace answers the bytes; the target is read where dL/dy was).  Checks: those of fz_run_block_loss_grad, in
 * its order, before a device is needed; a short workspace names fz_program_ring_grad_workspace.  For a graph without a deep line these
 * calls ARE the time-major fz_..._loss_grad_ calls: the same kernel, symbol, workspace and bits.  The kernel for a graph with one,
 * fz_adjoint_ring_loss_kernel_c<C>b<lanes per workgroup>_g<graph tag>, is a text of its own with the LDS bytes of the plain ring
 * kernel.  fz_run_block_loss_grad, its stream-major twin and the recording calls keep refusing graphs with a deep line. */
int fz_program_ring_loss_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out);
long fz_program_ring_loss_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
long fz_program_ring_loss_grad_source(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
int fz_run_block_ring_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream);

/* fz_run_block_far_grad, fz_run_block_far_loss_grad -- the two one-launch calls for graphs with delay lines DEEPER THAN 256 SAMPLES
 * (echoes, reverb combs, low plucked strings), whose rings live in HBM: a call family next to the fz_run_block_ring_grad family, as
 * that one stands next to fz_run_block_grad.  fz_grad_args and fz_loss_grad_args are taken unchanged; time-major frames (stream-major buffers:
 * fz_run_block_far_grad_stream_major below).
 *
 * THE CONTRACT.  Rules 1 - 4 of the ORDER OF OPERATIONS of fz_run_block_grad do not mention depth, and THE RULE of
 * fz_run_block_loss_grad applies as written: the bits are defined.  What is new is where a far line's adjoints lie in the caller's
 * state rows.  The `depth` state rows of such a line are ring slots and one more row holds the phase p (fz_program_lines): the value
 * u[q] of the line's source sits in slot (p0 + q) mod D for every position q, negative ones included, with p0 the phase before the
 * block -- before the block and, the phase being p0 + T then, after it.  Hence:
 *   state_grad, state0_grad: row row0 + k of a far line is the adjoint of SLOT k of the state after the block (state_grad) and before
 *     it (state0_grad).  The kernel's adjoint ring is loaded from state_grad and stored to state0_grad by the identity map, without a
 *     permutation, so state0_grad of block 2 passed as state_grad of block 1 gives the bits of one block of 2T, also where a block is
 *     shorter than the line.  The phase row of state_grad is never read; the phase row of state0_grad is written +0.0f.
 *   the phase is taken from `state` as the forward takes it -- uniform over the streams, the first active lane's value per wave -- and
 *     reduced modulo D: whatever the row holds, no access leaves the line's rows.
 * The bits do not depend on the checkpoint stride, the path (below), the lanes per workgroup or the stream count.
 *
 * Scope (fz_program_far_grad_check): fz_program_ring_grad_check's, plus float delay lines deeper than 256 samples.  Still refused,
 * with the reasons they have there: typed programs, float64 nodes, complex wires, modulators, LDS rings that fit no workgroup.  For a
 * graph without a far line these calls ARE the fz_..._ring_ calls: the same kernel, symbol, workspace and bits.  Every call of
 * the backward outside the far family keeps refusing a graph with a far line.
 *
 * The kernel, fz_adjoint_far_kernel_c<C>b<lanes>_g<tag> (fz_adjoint_far_loss_kernel_... under the loss), is the ring kernel's text
 * with its far mode compiled in (in every layout, and for the states kernel of a recording: one text, a compile-time switch, a
 * symbol of its own): register lines and LDS ring lines are what they are in the ring kernel.  Of a far line the forward sweep writes the source's value of every row into the tape
 * (the far lines are further tape lines) and reads its delayed values back from the tape rows it wrote -- for t < d from the caller's
 * slot (p0 + t - d) mod D.  STATIC RULE 1: a far read at least C rows old is requested with its chunk's x rows; a younger one is a
 * load of its own in front of its row.  The pending adjoints live in an adjoint ring in the workspace, one coalesced row per slot.
 * STATIC RULE 2: when every far read is at least C rows old and any two reads of one far line are at least C apart, no slot is touched
 * twice within a chunk: the chunk's slots are requested together with its x and tape rows, added to in registers and stored once
 * (the fast path: echoes, combs).  Otherwise every row loads, adds and stores in program order (the per-row path: a dependent memory
 * round trip per row).  The far lines use no LDS; lanes per workgroup: the ring rule's answer for the LDS ring lines alone, 256
 * without any.  C: checkpoint_rows, or for 0 the library default -- 16, halved while
 * C * (n_register_state + n_in + n_ring_reads + n_far_reads + (n_far_lines + n_far_reads)) exceeds 64: the ring rule with the far
 * reads among the ring reads, plus the slots a row of the fast path keeps in registers.
 * Workspace: (ceil(n_samples / C) * n_register_state + n_samples * (n_ring_lines + n_far_lines) + sum of the far depths) * n_streams
 * * 4 bytes; fz_program_far_grad_workspace answers it.  Checks: those of fz_run_block_grad / fz_run_block_loss_grad, in their order,
 * before a device is needed; a short workspace names fz_program_far_grad_workspace. */
int fz_program_far_grad_check(const fz_program* p);
int fz_program_far_grad_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t checkpoint_rows, uint64_t* bytes);
int fz_program_far_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out);
long fz_program_far_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
long fz_program_far_grad_source(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
int fz_run_block_far_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream);
int fz_program_far_loss_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out);
long fz_program_far_loss_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
long fz_program_far_loss_grad_source(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap);
int fz_run_block_far_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream);

/* fz_run_block_far_grad_stream_major, fz_run_block_far_loss_grad_stream_major -- the two one-launch calls of the
 * fz_run_block_far_grad family on STREAM-MAJOR buffers (a [batch, time] tensor as it lies).  The args structs are taken unchanged.
 *
 * THE CONTRACT IS A REFERENCE: every output bit is that of fz_run_block_far_grad / fz_run_block_far_loss_grad on the transposed
 * buffers.  Windows (rows_total, row0, n_samples) and the alignment of the buffers are those of fz_run_block_grad_stream_major: only
 * the rows of the window of in_grad (and of out) are written.  state, state_grad, state0_grad, params, the accumulators and the
 * workspace are [row][n_streams] in both layouts, so a far line's slot rows and phase row are those of fz_run_block_far_grad: the
 * phase is read from `state` and reduced modulo D, the phase row of state0_grad is written +0.0f, the phase row of state_grad is
 * never read, and blocks chain through state0_grad slot for slot as they do there.
 *
 * Scope: fz_program_far_grad_check's.  For a graph without a far line these calls ARE fz_run_block_ring_grad_stream_major /
 * fz_run_block_ring_loss_grad_stream_major (which for a graph without a ring line are the plain stream-major calls): the same
 * kernel, symbol, workspace and bits.  Checks: those of fz_run_block_ring_grad_stream_major, in its order, before a device is needed;
 * a short workspace names fz_program_far_grad_workspace, which answers both layouts.
 *
 * The kernel, fz_adjoint_far_sm_kernel_c<C>r<R>b<lanes>_g<tag> (fz_adjoint_far_loss_sm_kernel_...): the far kernel's sweeps, C, static
 * rules and paths; the frames move through a wave-private LDS patch of R rows as in the stream-major ring kernel.  The far lines use
 * no LDS: lanes per workgroup and R are the stream-major ring rule's answer for the LDS ring lines alone plus the patches, R
 * starting from half the ring kernels' longest patch and never below max(4, C) (a 1-in / 1-out graph without an LDS ring line at
 * C = 16: 256 lanes, R = 16, 36 864 bytes).  A graph whose LDS rings plus the shortest patch
 * fit no workgroup is refused with the bytes named.  fz_program_far_grad_*_for / fz_program_far_loss_grad_*_for inspect the kernel
 * of either layout (FZ_GRAD_TIME_MAJOR: what fz_program_far_grad_* answer).
 *
 * Recordings of such graphs on stream-major buffers: fz_run_recording_far_grad_for / fz_run_recording_far_loss_grad_for with
 * FZ_GRAD_STREAM_MAJOR, below (fz_run_recording_ring_grad_stream_major keeps refusing).  The forward of such graphs on stream-major
 * buffers: fz_run_block_far_stream_major (fz_run_block_stream_major keeps refusing).  Not built for graphs with a far line: double
 * or complex far lines. */
int fz_run_block_far_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0, uint32_t n_samples,
                                       void* hip_stream);
int fz_run_block_far_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                            uint32_t n_samples, void* hip_stream);
int fz_program_far_grad_resources_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, fz_kernel_resources* out);
long fz_program_far_grad_kernel_symbol_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
long fz_program_far_grad_source_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
int fz_program_far_loss_grad_resources_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, fz_kernel_resources* out);
long fz_program_far_loss_grad_kernel_symbol_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
long fz_program_far_loss_grad_source_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);

/* fz_run_block_ring_grad_stream_major, fz_run_block_ring_loss_grad_stream_major -- the two one-launch calls of the
 * fz_run_block_ring_grad family on STREAM-MAJOR buffers.  The args structs are taken unchanged.
 *
 * THE CONTRACT, by reference: the bits of fz_run_block_ring_grad (of fz_run_block_ring_loss_grad) on the transposed buffers -- the
 * layout does not change a bit -- and windows and alignment exactly as fz_run_block_grad_stream_major
 * (fz_run_block_loss_grad_stream_major): buffers [n_streams][rows_total][wire], the block is rows [row0, row0 + n_samples),
 * rows_total * n_in, rows_total * n_out, row0 * n_in and row0 * n_out multiples of 4 floats, rows of in_grad and of out outside the
 * window never written.  State, coefficient, accumulator rows and the workspace keep their [row][n_streams] layout.
 *
 * Scope: fz_program_ring_grad_check's.  Checkpoint stride and workspace: those of fz_run_block_ring_grad (fz_program_ring_grad_workspace
 * answers the bytes, unchanged).  Checks: those of fz_run_block_grad_stream_major / fz_run_block_loss_grad_stream_major, in their order,
 * before a device is needed; a short workspace names fz_program_ring_grad_workspace.  For a graph without a deep line these calls ARE
 * fz_run_block_grad_stream_major / fz_run_block_loss_grad_stream_major: the same kernel, symbol, workspace and bits.
 *
 * The kernels for a graph with a deep line, fz_adjoint_ring_sm_kernel_c<C>r<R>b<lanes>_g<tag> and
 * fz_adjoint_ring_loss_sm_kernel_c<C>r<R>b<lanes>_g<tag>, keep the rings AND the frame patches of R rows in LDS:
 * 4 * lanes * (ring samples + R * (n_in + n_out) + 4) bytes per workgroup.  Lanes and R are chosen together: R from the patch length
 * of fz_run_block_grad_stream_major halved down to max(4, C), lanes from 256 / 128 / 64; the first pair, in that order, that leaves
 * room for two workgroups in a compute unit's LDS, failing that the first that fits one.  Refused here alone (FZ_E_UNSUPPORTED): a
 * graph whose rings plus the shortest patch do not fit a workgroup at 64 lanes -- the reason names the bytes; a smaller
 * checkpoint_rows shortens the patch.  Not built: stream-major recordings of such graphs.
 * The inspection calls take (checkpoint_rows, layout) like their _grad_ twins. */
int fz_run_block_ring_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                        uint32_t n_samples, void* hip_stream);
int fz_run_block_ring_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                             uint32_t n_samples, void* hip_stream);
int fz_program_ring_grad_resources_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, fz_kernel_resources* out);
long fz_program_ring_grad_kernel_symbol_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
long fz_program_ring_grad_source_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
int fz_program_ring_loss_grad_resources_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, fz_kernel_resources* out);
long fz_program_ring_loss_grad_kernel_symbol_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);
long fz_program_ring_loss_grad_source_for(fz_program* p, uint32_t checkpoint_rows, uint32_t layout, char* buf, size_t cap);

/* fz_run_recording_grad, fz_run_recording_loss_grad -- the backward of a whole RECORDING of T rows in bounded workspace.
 *
 * THE CONTRACT (stated here once).  Every output bit -- in_grad, state0_grad, param_grad, const_grad, loss, out -- is that of the
 * one-launch call over the same T rows, fz_run_block_grad or fz_run_block_loss_grad (for FZ_GRAD_STREAM_MAJOR: their _stream_major
 * siblings over the window [row0, row0 + n_samples) of rows_total), whatever block_rows is; state_out, if not NULL, receives the
 * state after the last row with the bits of fz_run_block's state.  The arguments are those calls' (fz_grad_args / fz_loss_grad_args
 * over T rows, accumulators ADDED TO, state0_grad may be state_grad), plus the layout, block_rows and state_out.
 *
 * How: two-level checkpointing.  One launch of a block-start-states kernel runs the recording forward and stores only the state
 * before rows 0, B, 2B, ...; then the adjoint (or loss) kernel of the one-block calls is launched once per block, from the last
 * block to the first: block k covers rows [k B, min((k + 1) B, T)) with state = the k-th stored state, state_grad = the state0_grad
 * of the launch before it (in place) and the caller's accumulators throughout -- the chaining those calls document.  x is read
 * once more than by the one-launch call; the workspace holds ceil(T / B) + ceil(B / C) row sets instead of ceil(T / C).
 *
 * B: block_rows, or for block_rows == 0 the B that minimises ceil(B / C) + ceil(T / B): sqrt(T * C) rounded up to a multiple of
 * lcm(4, C), and B = T when that is not smaller than T.  A block_rows above T means one block of T rows.
 * fz_program_recording_block_rows answers the B a call will use.
 * WORKSPACE (the formula, stated here once): (ceil(T / B) + ceil(B / C)) * n_state * n_streams * 4 bytes, B as above, C the
 * checkpoint stride of fz_program_grad_workspace; fz_program_recording_workspace answers it.  One caller-owned buffer: the
 * block-start states [ceil(T / B)][n_state][n_streams] lie at its head, the workspace of the block launches behind them.
 *
 * Layout: FZ_GRAD_TIME_MAJOR -- frames [T][n_streams][wire], blocks are pointer offsets, so block_rows must be a multiple of 4 (the
 * 16-byte pointer rule of every launch; FZ_E_INVALID otherwise), row0 must be 0 and rows_total 0 or n_samples.
 * FZ_GRAD_STREAM_MAJOR -- buffers [n_streams][rows_total][wire], block k is the window row0 + k B, and every such window passes the
 * checks of fz_run_block_grad_stream_major (with more than one block: block_rows * n_in and block_rows * n_out multiples of 4).
 * The state and the workspace of a block launch are the library's own [row][n_streams] rows of the caller's workspace, touched in
 * 4-byte accesses per lane like the checkpoint rows of any launch: the 16-byte rule is asked of the caller's pointers only.
 * Checks, all before a device is needed: the refusals of fz_program_grad_check, unchanged; those of the one-launch call over the T
 * rows (state_out counted as an output) with this call's workspace size; those of every block launch; n_samples < 2^31; with more
 * than one block and delay lines, state0_grad must not be NULL (the blocks chain through it).  n_streams == 0 or n_samples == 0:
 * FZ_OK, nothing is touched.  A graph without delay lines launches no states kernel; a graph without inputs reads no frames.
 * Asynchronous on hip_stream like the one-block calls.
 *
 * The states kernel is a kernel text of its own per layout, fz_states_kernel_u<U>b<lanes>_g<tag> and
 * fz_states_sm_kernel_u<U>r<R>b<lanes>_g<tag> (U rows per unrolled group; R rows of the LDS patch x moves through, x only:
 * lds_bytes = 4 waves * 64 * (R * n_in + 4) * 4; none for a graph without input wires, and none for one without delay lines, whose
 * kernel has nothing to store and is never launched); fz_program_states_* inspect it like their _grad_ twins. */
int fz_program_recording_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows,
                                   uint32_t layout, uint64_t* bytes);
int fz_program_recording_block_rows(const fz_program* p, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows, uint32_t* rows);
int fz_run_recording_grad(fz_program* p, const fz_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                          uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream);
int fz_run_recording_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                               uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream);
int fz_program_states_resources(fz_program* p, uint32_t layout, fz_kernel_resources* out);
long fz_program_states_kernel_symbol(fz_program* p, uint32_t layout, char* buf, size_t cap);
long fz_program_states_source(fz_program* p, uint32_t layout, char* buf, size_t cap);

/* fz_run_recording_ring_grad, fz_run_recording_ring_loss_grad -- the backward of a whole recording of a graph with delay lines deeper
 * than 8 samples, in bounded workspace: to fz_run_block_ring_grad / fz_run_block_ring_loss_grad what fz_run_recording_grad /
 * fz_run_recording_loss_grad are to the one-block calls, on time-major frames (stream-major buffers: their _stream_major siblings, below).
 *
 * The contract is the one stated above, read with the ring calls as the one-launch calls: every output bit -- in_grad, state0_grad,
 * param_grad, const_grad, loss, out -- is that of fz_run_block_ring_grad / fz_run_block_ring_loss_grad over the same T rows, whatever
 * block_rows is; state_out, if not NULL, receives the state after row T-1 with the bits of fz_run_block's state.  fz_grad_args and
 * fz_loss_grad_args are taken unchanged, the accumulators are ADDED TO, state0_grad may be state_grad.  No new arithmetic rule: two
 * ring blocks chain bitwise, also where a block is shorter than a line is deep (fz_run_block_ring_grad says so).
 *
 * Scope: that of fz_program_ring_grad_check.  For a graph without a deep line these calls ARE the FZ_GRAD_TIME_MAJOR
 * fz_run_recording_grad / fz_run_recording_loss_grad: the same states kernel, B, workspace and bits.  fz_run_recording_*,
 * fz_program_recording_workspace and fz_program_states_* keep refusing graphs with deep lines.
 *
 * How: one launch of the RING STATES kernel writes starts[ceil(T / B)][n_state][n_streams] at the head of the workspace (and state_out);
 * then the ring adjoint or ring loss kernel is launched, unchanged, per block from the last to the first, with state = starts[k] and
 * state_grad = the state0_grad of the launch before it.  The states kernel keeps each deep line as a value ring in LDS (the ring
 * kernel's sweep 1 without the tape) and reads a line's D values back out of LDS in the caller's row order at every block start.
 *
 * B: block_rows, capped at T; for block_rows == 0 the least B with B^2 (n_register_state + C n_ring_lines) >= T n_state C -- the
 * continuous minimiser of ceil(T / B) n_state + ceil(B / C) n_register_state + B n_ring_lines, the rows kept per stream -- rounded up
 * to a multiple of max(4, C), and B = T when that is not smaller than T (n_register_state: the state floats of the lines of depth
 * <= 8; C: the ring kernel's checkpoint stride).  Without a deep line this is the rule above.  fz_program_ring_recording_block_rows
 * answers the B a call will use.
 * WORKSPACE: ceil(T / B) * n_state * n_streams * 4 bytes plus fz_program_ring_grad_workspace(n_streams, B, C);
 * fz_program_ring_recording_workspace answers it.
 *
 * Checks, all before a device is needed and in this order: the refusals of fz_program_ring_grad_check; block_rows a multiple of 4;
 * n_samples < 2^31; those of the one-launch ring call over the T rows (state_out counted as an output) with this call's workspace
 * size; those of every block launch; with more than one block, state0_grad not NULL.  n_streams == 0 or n_samples == 0: FZ_OK,
 * nothing is touched.  Asynchronous on hip_stream.
 *
 * The ring states kernel is a kernel of its own, fz_states_ring_kernel_u<U>b<lanes>_g<tag> (U rows per unrolled group; the
 * lanes and lds_bytes of the ring adjoint kernel); fz_program_ring_states_* inspect it like fz_program_states_*. */
int fz_program_ring_recording_block_rows(const fz_program* p, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows, uint32_t* rows);
int fz_program_ring_recording_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows,
                                        uint64_t* bytes);
int fz_run_recording_ring_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows, float* state_out,
                               void* hip_stream);
int fz_run_recording_ring_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows,
                                    float* state_out, void* hip_stream);
int fz_program_ring_states_resources(fz_program* p, fz_kernel_resources* out);
long fz_program_ring_states_kernel_symbol(fz_program* p, char* buf, size_t cap);
long fz_program_ring_states_source(fz_program* p, char* buf, size_t cap);

/* fz_run_recording_ring_grad_stream_major, fz_run_recording_ring_loss_grad_stream_major -- the same on STREAM-MAJOR buffers
 * [n_streams][rows_total][wire], the recording the window of rows [row0, row0 + n_samples): a batch of recordings lying as
 * [batch, time] is taken as it lies, without a transposed copy of the frames.
 *
 * THE CONTRACT IS A REFERENCE.  Every output bit -- in_grad, state0_grad, param_grad, const_grad, loss, out -- is that of
 * fz_run_recording_ring_grad / fz_run_recording_ring_loss_grad on the transposed buffers (and so that of the one-launch
 * fz_run_block_ring_grad_stream_major / fz_run_block_ring_loss_grad_stream_major over the same window), whatever block_rows is.
 * Windows, alignment and the rows outside the window, which are never written, are those of fz_run_recording_grad with
 * FZ_GRAD_STREAM_MAJOR: block k is the window row0 + k B, and every such window passes the checks of
 * fz_run_block_ring_grad_stream_major (rows_total, row0 and, with more than one block, block_rows times n_in and n_out multiples of
 * 4 floats).  state_out, if not NULL, receives the state after the window's last row with the bits of fz_run_block's state.
 * fz_grad_args and fz_loss_grad_args are taken unchanged.
 *
 * B and the workspace: fz_program_ring_recording_block_rows and fz_program_ring_recording_workspace answer both layouts -- C, the
 * tape, the checkpoints and the block-start states do not depend on the layout (the workspace query asks for a block_rows that is a
 * multiple of 4 in either layout).
 *
 * Scope: that of fz_program_ring_grad_check, plus the LDS refusals of the two stream-major kernels, whose rings share the
 * workgroup's LDS with the patches the frames move through: a graph whose block kernel fz_run_block_ring_grad_stream_major refuses
 * at the default stride is refused here with that reason and taken at a checkpoint_rows that fits.  For a graph without a deep line
 * these calls ARE fz_run_recording_grad / fz_run_recording_loss_grad with FZ_GRAD_STREAM_MAJOR: the same states kernel, B, workspace
 * and bits.  fz_run_recording_grad with FZ_GRAD_STREAM_MAJOR keeps refusing graphs with deep lines, and the time-major
 * fz_run_recording_ring_* keep having no window.
 *
 * Checks, all before a device is needed and in this order: the refusals of fz_program_ring_grad_check; the states kernel's LDS;
 * n_samples < 2^31; the block kernel's LDS; those of the one-launch stream-major ring call over the window (state_out counted as an
 * output) with this call's workspace size -- a short workspace names fz_program_ring_recording_workspace; with more than one block,
 * state0_grad not NULL; those of every block launch.  n_streams == 0 or n_samples == 0: FZ_OK, nothing is touched.  Asynchronous on
 * hip_stream.
 *
 * The states kernel is a kernel of its own, fz_states_ring_sm_kernel_u<U>r<R>b<lanes>_g<tag>: U rows per unrolled group as for
 * every states kernel; x moves through a wave-private LDS patch of R rows next to the value rings, lds_bytes =
 * 4 * lanes * (ring samples + R * n_in + 4) (no patch for a graph without input wires).  R runs over twice the R of
 * fz_states_sm_kernel, halved down to max(4, U); per R the lanes over 256 / 128 / 64; the first pair that fits a compute unit's LDS
 * twice wins, failing that the first that fits once, otherwise FZ_E_UNSUPPORTED naming the bytes.  The _for calls inspect the ring
 * states kernel of a layout (FZ_GRAD_TIME_MAJOR: fz_program_ring_states_*). */
int fz_run_recording_ring_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                            uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream);
int fz_run_recording_ring_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                                 uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream);
int fz_program_ring_states_resources_for(fz_program* p, uint32_t layout, fz_kernel_resources* out);
long fz_program_ring_states_kernel_symbol_for(fz_program* p, uint32_t layout, char* buf, size_t cap);
long fz_program_ring_states_source_for(fz_program* p, uint32_t layout, char* buf, size_t cap);

/* fz_run_recording_far_grad, fz_run_recording_far_loss_grad -- fz_run_recording_ring_grad / fz_run_recording_ring_loss_grad for
 * graphs with delay lines DEEPER THAN 256 SAMPLES (rings in HBM): the third pair of members of the far call family, the gradient of
 * a whole recording of T time-major rows in a workspace that does not hold a tape of T rows per far line.
 *
 * NO NEW RULE.  Every output bit -- in_grad, state0_grad, param_grad, const_grad, loss, out -- is that of fz_run_block_far_grad /
 * fz_run_block_far_loss_grad over the same T rows, whatever block_rows is: far blocks chain bitwise through state0_grad slot for
 * slot, also where a block is shorter than a line is deep (fz_run_block_far_grad says so).  starts[k], at the head of the workspace,
 * and state_out, if not NULL, have the bits of fz_run_block's state after k B / T rows, the far lines' rows included: the value u[q]
 * in slot (p0 + q) mod D, the phase row (p0 + k B) mod D / (p0 + T) mod D as the forward writes it.  fz_grad_args and
 * fz_loss_grad_args are taken unchanged, the accumulators are ADDED TO, state0_grad may be state_grad.
 *
 * Scope: that of fz_program_far_grad_check.  For a graph without a line deeper than 256 samples these calls ARE
 * fz_run_recording_ring_grad / fz_run_recording_ring_loss_grad (and so, without a deep line at all, the FZ_GRAD_TIME_MAJOR
 * fz_run_recording_grad / fz_run_recording_loss_grad): the same states kernel, B, workspace and bits.  fz_run_recording_*,
 * fz_run_recording_ring_*, fz_program_ring_recording_* and fz_program_ring_states_* keep refusing graphs with such lines.
 * Time-major frames; stream-major buffers: the _for calls below.
 *
 * How: one launch of the FAR STATES kernel writes starts[ceil(T / B)][n_state][n_streams] (and state_out); then the far adjoint or
 * far loss kernel is launched, unchanged, per block from the last to the first, with state = starts[k] and state_grad = the
 * state0_grad of the launch before it.  The far states kernel is the ring states kernel with sweep 1 of the far adjoint kernel as
 * its step.  It keeps a far line as a WORKING VALUE RING in the caller's own slot format in the rows of the workspace behind
 * `starts` -- rows of the block workspace, which no launch has used yet, so the workspace does not grow --, filled once from
 * `state` by the identity map; per row one load per far read and one store per far line, no tape; at a block start a line's D slots
 * are copied row for row.  STATIC RULE: the rows go in groups of U, and a far read at a delay of at least 2 U -- its slot was
 * written before the next group's x rows are requested -- is requested with them; a younger read is a load of its own in front of
 * its row (same-lane program order).  HBM bytes per stream-sample: 4 n_in + 4 n_far_lines + 4 n_far_reads + (4 n_state + 4 * sum of
 * the far depths) / B.
 *
 * B: block_rows, capped at T; for block_rows == 0 the least B with B^2 (n_register_state + C (n_ring_lines + n_far_lines)) >=
 * T n_state C, rounded up to a multiple of max(4, C), and B = T when that is not smaller than T -- the ring rule with the far lines
 * among the tape lines (C: the far kernel's checkpoint stride; n_state counts a far line's D slots and its phase row, so a block
 * start costs D + 1 rows per far line and the blocks are long).  The rows kept per stream are ceil(T / B) n_state + ceil(B / C)
 * n_register_state + B (n_ring_lines + n_far_lines) + the sum of the far depths.  Without a far line this is the ring rule.
 * fz_program_far_recording_block_rows answers the B a call will use.
 * WORKSPACE: ceil(T / B) * n_state * n_streams * 4 bytes plus fz_program_far_grad_workspace(n_streams, B, C);
 * fz_program_far_recording_workspace answers it.
 *
 * Checks, all before a device is needed and in this order: the refusals of fz_program_far_grad_check; block_rows a multiple of 4;
 * n_samples < 2^31; those of the one-launch far call over the T rows (state_out counted as an output) with this call's workspace
 * size -- a short workspace names fz_program_far_recording_workspace; those of every block launch; with more than one block,
 * state0_grad not NULL.  n_streams == 0 or n_samples == 0: FZ_OK, nothing is touched.  Asynchronous on hip_stream.
 *
 * The far states kernel is a kernel of its own, fz_states_far_kernel_u<U>b<lanes>_g<tag> (U rows per unrolled group, at most 8; the
 * lanes and lds_bytes of the far adjoint kernel: the LDS ring lines' alone); fz_program_far_states_* inspect it like
 * fz_program_ring_states_*. */
int fz_program_far_recording_block_rows(const fz_program* p, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows, uint32_t* rows);
int fz_program_far_recording_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows,
                                       uint64_t* bytes);
int fz_run_recording_far_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows, float* state_out,
                              void* hip_stream);
int fz_run_recording_far_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows,
                                   float* state_out, void* hip_stream);
int fz_program_far_states_resources(fz_program* p, fz_kernel_resources* out);
long fz_program_far_states_kernel_symbol(fz_program* p, char* buf, size_t cap);
long fz_program_far_states_source(fz_program* p, char* buf, size_t cap);

/* fz_run_recording_far_grad_for, fz_run_recording_far_loss_grad_for -- the same with the layout as an ARGUMENT, the argument list of
 * fz_run_recording_grad / fz_run_recording_loss_grad: with FZ_GRAD_STREAM_MAJOR a graph with delay lines in HBM is fitted to a batch
 * of recordings lying as [batch, time], buffers [n_streams][rows_total][wire], the recording the window of rows
 * [row0, row0 + n_samples), without a transposed copy of the frames.  With FZ_GRAD_TIME_MAJOR the calls ARE fz_run_recording_far_grad /
 * fz_run_recording_far_loss_grad (row0 0 and rows_total 0 or n_samples: time-major frames have no window): the same checks, kernels
 * and bits.
 *
 * THE CONTRACT IS A REFERENCE.  Every output bit -- in_grad, state0_grad, param_grad, const_grad, loss, out -- is that of
 * fz_run_recording_far_grad / fz_run_recording_far_loss_grad on the transposed buffers (and so that of the one-launch
 * fz_run_block_far_grad_stream_major / fz_run_block_far_loss_grad_stream_major over the same window), whatever block_rows is.
 * starts[k] at the head of the workspace and state_out, if not NULL, have the bits of fz_run_block's state, the far lines' slots
 * (u[q] in slot (p0 + q) mod D) and phase rows included.  Windows, alignment and the rows outside the window, which are never
 * written, are those of fz_run_recording_grad with FZ_GRAD_STREAM_MAJOR: block k is the window row0 + k B, and every such window
 * passes the checks of fz_run_block_far_grad_stream_major.  fz_grad_args and fz_loss_grad_args are taken unchanged.
 *
 * B and the workspace: fz_program_far_recording_block_rows and fz_program_far_recording_workspace answer both layouts -- C, the
 * tape, the adjoint ring, the checkpoints and the block-start states do not depend on the layout (the workspace query asks for a
 * block_rows that is a multiple of 4 in either layout).
 *
 * Scope: that of fz_program_far_grad_check, plus the LDS refusals of the two stream-major kernels.  For a graph without a line deeper
 * than 256 samples the stream-major calls ARE fz_run_recording_ring_grad_stream_major / fz_run_recording_ring_loss_grad_stream_major
 * (and so, without a deep line at all, fz_run_recording_grad / fz_run_recording_loss_grad with FZ_GRAD_STREAM_MAJOR): the same states
 * kernel, B, workspace and bits.  Every other recording call keeps refusing graphs with far lines; double or complex far lines stay
 * refused.
 *
 * Checks, all before a device is needed, in the order of fz_run_recording_ring_grad_stream_major: the refusals of
 * fz_program_far_grad_check; the states kernel's LDS; n_samples < 2^31; the block kernel's LDS; those of the one-launch stream-major
 * far call over the window (state_out counted as an output) with this call's workspace size -- a short workspace names
 * fz_program_far_recording_workspace; with more than one block, state0_grad not NULL; those of every block launch.  n_streams == 0
 * or n_samples == 0: FZ_OK, nothing is touched.  Asynchronous on hip_stream.
 *
 * The stream-major far states kernel, fz_states_far_sm_kernel_u<U>r<R>b<lanes>_g<tag>, is the stream-major ring states kernel with
 * what the far mode adds to the time-major one: the working value ring of a far line in the rows of the workspace behind `starts`,
 * one load per far read and one store per far line and row, the reads at a delay of at least 2 U requested one group of U rows
 * ahead, a line's D slots copied row for row at a block start.  x moves through a wave-private LDS patch of R rows; the far lines
 * take no LDS: lds_bytes = 4 * lanes * (LDS ring samples + R * n_in + 4).  R runs over the R of fz_states_sm_kernel (never below
 * max(4, U)) -- half the ring states kernel's: a far kernel waits on rows in HBM and needs waves more than a longer run -- halved
 * down to max(4, U); per R the lanes over 256 / 128 / 64, as for the ring states kernel (a 1-in graph without an LDS ring line:
 * 256 lanes, R = 32, 36 864 bytes).  HBM bytes per stream-sample: those of the time-major far states kernel.  The _for inspection
 * calls answer for a layout (FZ_GRAD_TIME_MAJOR: fz_program_far_states_*). */
int fz_run_recording_far_grad_for(fz_program* p, const fz_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                  uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream);
int fz_run_recording_far_loss_grad_for(fz_program* p, const fz_loss_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total,
                                       uint32_t row0, uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream);
int fz_program_far_states_resources_for(fz_program* p, uint32_t layout, fz_kernel_resources* out);
long fz_program_far_states_kernel_symbol_for(fz_program* p, uint32_t layout, char* buf, size_t cap);
long fz_program_far_states_source_for(fz_program* p, uint32_t layout, char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------
 * 16-bit PCM frames.  fz_run_block_pcm16 is fz_run_block for a block whose frames are int16 on one side or on both: the caller
 * sends and receives 2 bytes per sample instead of 4, the conversions happen in the kernel.
 *
 * THE CONVERSION RULE (stated here once; the kernel, the host path and the tests follow it):
 *   in    x = (float)q * 2^-15 for q in [-32768, 32767].  Exact: no rounding, and -32768 gives -1.0f.
 *   out   r = y * 32768.0f, ONE float32 multiplication (exact unless it overflows, and an overflow saturates anyway); then, in this
 *         order:  y NaN -> 0;  r >= 32767.0f -> 32767;  r <= -32768.0f -> -32768;  else r rounded to the nearest integer, ties to even.
 *   No dither, no noise shaping.
 * Between the two conversions the arithmetic is that of fz_run_block (one IEEE float32 rounding per graph node, no FMA, correctly
 * rounded division and square root, denormals kept): a float32 output equals fz_run_block on the converted input bit for bit, an
 * int16 output is the rule applied to that float32 output.  No tolerance is involved anywhere.
 *
 * Frames are time-major, in [n_samples][n_streams][n_in] and out [n_samples][n_streams][n_out], each side int16_t (FZ_FRAMES_I16) or
 * float (FZ_FRAMES_F32) as in_type / out_type say; state and params are those of fz_run_block -- the state layout does not depend
 * on the frame type, so float32 blocks and PCM blocks chain on one state buffer.  Any n_streams >= 1: where n_streams * wires is odd
 * on an int16 side, its rows start off the dword grid and a second instantiation of the kernel (2-byte accesses) runs.
 *
 * Argument checks as for fz_run_block, all made before the device is needed: device pointers 16-byte aligned; a pointer NULL iff its
 * width is 0; an unknown frame type is FZ_E_INVALID; float32 on both sides is FZ_E_INVALID (that block is fz_run_block); an empty
 * block is FZ_OK and touches nothing; a row of 4 GiB or more is FZ_E_UNSUPPORTED.  `in` and `out` may be the SAME buffer when both
 * sides are int16 and n_in == n_out (in place); any other overlap of the two is FZ_E_INVALID.
 *
 * Scope: fz_compile programs that are float32 throughout and whose delay lines live in registers (max_delay <= 8).  Typed programs,
 * float64 nodes, complex wires, modulators and delay lines in LDS or HBM rings are FZ_E_UNSUPPORTED, fz_last_error() names which
 * (fz_program_pcm16_check asks without a device).
 *
 * STREAM-MAJOR buffers -- a [batch, time] int16 tensor as it lies: fz_run_block_pcm16_stream_major is fz_run_block_stream_major with
 * a frame type per side.  in [n_streams][rows_total][n_in], out [n_streams][rows_total][n_out]; the block is the window of rows
 * [row0, row0 + n_samples), rows outside it are never written.  Same rule, same state: float32 blocks, time-major PCM blocks and
 * stream-major PCM blocks chain on one state buffer, and a float32 output equals fz_run_block_stream_major on the converted input
 * bit for bit.  n_samples is free.  THE ALIGNMENT RULE: frames travel as 16-byte pieces, so every stream's buffer and the window's
 * first row start on that grid -- rows_total * wires and row0 * wires are multiples of 8 on an int16 side and of 4 on a float32
 * side, else FZ_E_INVALID (fz_last_error() names the side and the multiple).  Checks, in this order and before a device is needed:
 * the scope above; the frame types; an empty block is FZ_OK; row0 + n_samples <= rows_total; the alignment rule; pointers 16-byte
 * aligned, `in` / `out` NULL iff that side has no wires; in == out allowed with int16 on both sides and n_in == n_out, every other
 * overlap of the two whole buffers FZ_E_INVALID; 2^30 streams or more FZ_E_UNSUPPORTED.
 *
 * Not built: stream-tiled PCM frames, windows of time-major PCM frames, 24-bit and float16 frames, dither, PCM in the backward,
 * fz_program_tune for these kernels (their plans are static).
 * ---------------------------------------------------------------------------------------- */
enum { FZ_FRAMES_F32 = 0, FZ_FRAMES_I16 = 1 };
/* FZ_OK, or FZ_E_UNSUPPORTED with the reason in fz_last_error(); host only */
int  fz_program_pcm16_check(const fz_program* p);
int  fz_run_block_pcm16(fz_program* p, const void* in, void* out, float* state, const float* params,
                        uint64_t n_streams, uint32_t n_samples, uint32_t in_type, uint32_t out_type, void* hip_stream);
/* The kernel a block of (in_type, out_type, n_streams) runs (n_streams 0: 2^20), without a device: its registers and scratch
 * (`unroll` = rows per chunk), its symbol fz_pcm16_kernel_i<0|1>o<0|1>p<streams per lane>u<rows per chunk>b<lanes per workgroup>[h][m]_g<graph tag>
 * -- i / o: that side is int16; h: 2-byte accesses (int16 rows off the dword grid); m: stores that let L2 merge sectors (output
 * rows off the 64-byte grid) -- and its whole source.  The stream count matters only through those two letters. */
int  fz_program_pcm16_resources(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams, fz_kernel_resources* out);
long fz_program_pcm16_kernel_symbol(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams, char* buf, size_t cap);
long fz_program_pcm16_source(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams, char* buf, size_t cap);
int  fz_run_block_pcm16_stream_major(fz_program* p, const void* in, void* out, float* state, const float* params,
                                     uint64_t n_streams, uint32_t rows_total, uint32_t row0, uint32_t n_samples,
                                     uint32_t in_type, uint32_t out_type, void* hip_stream);
/* The kernel a stream-major block of (in_type, out_type) runs, without a device: its registers, scratch and LDS (`unroll` = rows per
 * chunk; lds_bytes = 64 * (rows * (n_in * ie + n_out * oe) + 16), ie / oe = 2 for int16 and 4 for float32), its symbol
 * fz_pcm16_sm_kernel_i<0|1>o<0|1>u<rows per chunk>b<lanes per workgroup>_g<graph tag>, and its whole source. */
int  fz_program_pcm16_stream_major_resources(fz_program* p, uint32_t in_type, uint32_t out_type, fz_kernel_resources* out);
long fz_program_pcm16_stream_major_kernel_symbol(fz_program* p, uint32_t in_type, uint32_t out_type, char* buf, size_t cap);
long fz_program_pcm16_stream_major_source(fz_program* p, uint32_t in_type, uint32_t out_type, char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------
 * Delay lines deeper than 256 samples on STREAM-MAJOR buffers, forward.  fz_run_block_far_stream_major is fz_run_block_stream_major
 * for a graph whose deepest lines keep their rings in HBM: in [n_streams][rows_total][n_in], out [n_streams][rows_total][n_out],
 * float32, a [batch, time] tensor as it lies; the block is the window of rows [row0, row0 + n_samples), rows outside it are never
 * touched.  state and params are fz_run_block's ([row][n_streams]); the far rings are read and written where they are, in the rows
 * of `state`.  The bits of `out` and of every state row -- register rows, LDS-ring rows, far slots, phase rows -- are fz_run_block's
 * on the transposed frames, so blocks of either call chain on one state buffer.  One launch on hip_stream, no host synchronisation.
 * For a graph WITHOUT a line deeper than 256 samples the call is fz_run_block_stream_major with a NULL variant: same kernel, same
 * bits, same refusals.
 *
 * The kernel (fz_kernel_far_sm.hip.inc): one stream per lane; whole chunks of R rows travel as 16-byte pieces through a wave-private
 * LDS patch, the rows behind the last whole chunk run one step at a time.  Every step appends one row per far line; inside whole
 * chunks a far read comes from a register buffer requested one group of G unrolled rows ahead, behind them from a load in front of
 * its row.  THE GROUP RULE: a read requested a group ahead must touch no slot that the group in between writes, 2 G <=
 * far_min_read (the youngest read served from a ring in HBM, at least 9); G is the largest power of two not above
 * min(16, far_min_read / 2), halved, not below 4, while the two read buffers, 2 G n_far_reads registers, pass 64.  THE LDS RULE:
 * delay lines of 9 .. 256 samples of the same graph keep their rings in LDS, ring[slot][lane]; rings and patches share the
 * workgroup's LDS, 4 n_lds_slots lanes + (lanes / 64) * 64 * (4 R (n_in + n_out) + 16) bytes.  R runs from the shortest power of two,
 * at least 16, at which one stream's run in the wider frame is 128 bytes (32 rows for one wire) down to 16, per R the lanes over
 * 256, 128, 64: the first pair that fits 160 KiB twice, failing that once.
 *
 * Checks, in this order and before a device is needed: rows_total > 0; the scope (fz_program_far_stream_major_check asks without a
 * device); an empty block is FZ_OK; row0 + n_samples <= rows_total; the alignment rule of fz_run_block_stream_major (rows_total *
 * wires and row0 * wires multiples of 4 floats per side, fz_last_error() names the side); a pointer the graph needs is not NULL
 * (named); pointers 16-byte aligned; 2^30 streams or more FZ_E_UNSUPPORTED.  `in` and `out` must not overlap.
 *
 * Scope: fz_compile programs with float far lines.  FZ_E_UNSUPPORTED with the reason in fz_last_error(): fz_compile_typed programs,
 * complex wires, sample-rate modulators, double or complex far lines, a graph whose LDS rings plus the shortest patch fit no
 * workgroup (the bytes named).  Frames are float32: the call has no float64-frames form (FZ_VF_OUT_F64 belongs to a variant, and
 * this call takes none); float64 nodes evaluate in double and narrow to the float32 frame as in fz_run_block.
 * Everything else keeps refusing these graphs on stream-major buffers: fz_run_block_stream_major, fz_bank_process_stream_major,
 * fz_bank_process_host_stream_major, the PCM calls, fz_program_tune.
 * Not built: double or complex far lines, the bank, PCM frames and fz_program_tune on this path (its plan is static).
 * ---------------------------------------------------------------------------------------- */
/* FZ_OK, or FZ_E_UNSUPPORTED with the reason in fz_last_error(); host only */
int  fz_program_far_stream_major_check(const fz_program* p);
int  fz_run_block_far_stream_major(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
                                   uint32_t rows_total, uint32_t row0, uint32_t n_samples, void* hip_stream);
/* The kernel the call runs, without a device: its registers, scratch and LDS (`unroll` = G; lds_bytes by the LDS rule above), its
 * symbol fz_far_sm_kernel_g<G>r<R>b<lanes per workgroup>_g<graph tag>, and its whole source.  A graph without a far line: what
 * fz_program_kernel_resources / _kernel_symbol / fz_program_source answer for {0, 0, 0, FZ_VF_STREAM_MAJOR}. */
int  fz_program_far_stream_major_resources(fz_program* p, fz_kernel_resources* out);
long fz_program_far_stream_major_kernel_symbol(fz_program* p, char* buf, size_t cap);
long fz_program_far_stream_major_source(fz_program* p, char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------
 * fz_bank -- device-resident closure state for n_streams streams: the `state_` member of
 * stateful_lambda (flowz.hpp:1190-1191).  clone == copying the closure (snapshot, :1206).
 * The *_host entry points stage through device memory (H2D, kernel, D2H, synchronous); they
 * exist so that the reference's per-sample call protocol works unchanged on top.
 * ---------------------------------------------------------------------------------------- */
typedef struct fz_bank fz_bank;

int  fz_bank_create(fz_program* p, uint64_t n_streams, fz_bank** out);   /* zero state        */
int  fz_bank_clone(const fz_bank* b, fz_bank** out);
void fz_bank_destroy(fz_bank* b);
int  fz_bank_reset(fz_bank* b);                                          /* state := 0        */
int  fz_bank_set_params_host(fz_bank* b, const float* params /* [n_param][n_streams] */);
float* fz_bank_state_device(fz_bank* b);                                 /* [n_state][n_streams] */
int  fz_bank_process(fz_bank* b, const float* in_dev, float* out_dev, uint32_t n_samples,
                     const fz_variant* v, void* hip_stream);
/* fz_bank_process with stream-tiled frames (see fz_run_block_tiled) */
int  fz_bank_process_tiled(fz_bank* b, const float* in_dev, float* out_dev, uint32_t n_samples,
                           uint32_t tile_streams, const fz_variant* v, void* hip_stream);
/* fz_run_block_stream_major on the bank's state: in [n_streams][rows_total][n_in], out alike */
int  fz_bank_process_stream_major(fz_bank* b, const float* in_dev, float* out_dev, uint32_t rows_total, uint32_t row0,
                                  uint32_t n_samples, const fz_variant* v, void* hip_stream);
/* Control-rate modulation (the std::ref terminals of flowz/README.md:42-61 at block rate): the
 * rows_total samples of the frame buffers are processed in blocks of block_len samples, block k with the
 * per-stream coefficient set params_blocks[k] (device, [n_blocks][n_param][n_streams]; NULL: the bank's
 * own set).  ceil(rows_total / block_len) back-to-back launches, state carried.                          */
int  fz_bank_process_blocks(fz_bank* b, const float* in_dev, float* out_dev, uint32_t rows_total, uint32_t block_len,
                            const float* params_blocks, uint32_t tile_streams, const fz_variant* v, void* hip_stream);
/* fz_program_tune on the bank's own state and per-stream coefficients (the state advances: fz_bank_reset) */
int  fz_bank_tune(fz_bank* b, const float* in_dev, float* out_dev, uint32_t n_samples, uint32_t tile_streams,
                  void* hip_stream, fz_variant* chosen, float* chosen_ms);
int  fz_bank_process_host(fz_bank* b, const float* in_host, float* out_host, uint32_t n_samples);
/* host buffers in the reference's own calling convention: one contiguous sample buffer per stream,
 * in [n_streams][n_samples][n_in] -> out [n_streams][n_samples][n_out] (2-D copies of time chunks, the
 * stream-major kernel, the same three-stream pipeline)                                               */
int  fz_bank_process_host_stream_major(fz_bank* b, const float* in_host, float* out_host, uint32_t n_samples);
/* the same with float64 result frames (FZ_VF_OUT_F64): what a closure with double literals returns
 * in the reference (tuple<double>, flowz.hpp:1225-1229 with the ResultType of test/tests.cpp:201) */
int  fz_bank_process_host_f64(fz_bank* b, const float* in_host, double* out_host, uint32_t n_samples);
/* fz_run_block_pcm16 on the bank's state (device frames, asynchronous on hip_stream), and the host path of fz_bank_process_host for a
 * caller that holds interleaved 16-bit PCM: int16 frames in, int16 frames out, through int16 staging buffers, the same time chunks
 * and the same three streams -- half the PCIe bytes in each direction */
int  fz_bank_process_pcm16(fz_bank* b, const void* in_dev, void* out_dev, uint32_t n_samples, uint32_t in_type, uint32_t out_type,
                           void* hip_stream);
int  fz_bank_process_host_pcm16(fz_bank* b, const int16_t* in_host, int16_t* out_host, uint32_t n_samples);
/* fz_run_block_pcm16_stream_major on the bank's state, and fz_bank_process_host_stream_major for a caller that holds [batch, time]
 * int16: host buffers in [n_streams][n_samples][n_in] -> out [n_streams][n_samples][n_out], any n_samples (the 2-D copies take any
 * host pitch), time chunks of whole 32 rows in compact int16 device patches, the same three streams */
int  fz_bank_process_pcm16_stream_major(fz_bank* b, const void* in_dev, void* out_dev, uint32_t rows_total, uint32_t row0,
                                        uint32_t n_samples, uint32_t in_type, uint32_t out_type, void* hip_stream);
int  fz_bank_process_host_pcm16_stream_major(fz_bank* b, const int16_t* in_host, int16_t* out_host, uint32_t n_samples);

/* ------------------------------------------------------------------------------------------
 * Device utilities used by the measurement harness (bench.py) and tests.
 * ---------------------------------------------------------------------------------------- */
int fz_device_count(void);                /* 0 when no GPU is visible                          */
/* synthetic frames (t, s, w) = unit(hash32(seed, (stream0+s)*n_wires + w, t0+t)) in [-1,1), stored
 * time-major (tile_streams == 0) or stream-tiled as fz_run_block_tiled expects                */
int fz_synth_fill(float* dst_dev, uint64_t n_streams, uint32_t n_samples, uint32_t n_wires,
                  uint32_t seed, uint64_t stream0, uint64_t t0, uint32_t tile_streams, void* hip_stream);
/* Per-stream biquad coefficients on the device: the RBJ low-pass equations of the reference's
 * reactive_equations/reactive_filter_coeff.cpp:38-58 with its parameter types (every PARAMETER is
 * float, the literals `1.`, `2.` are double):
 *     w0 = two_pi*freq/sr (float)   cosw0 = cos(w0)   alpha = sin(w0)/(2.*Q)
 *     b0 = (1.-cosw0)/2.   b1 = 1.-cosw0   b2 = (1.-cosw0)/2.   a0 = 1.+alpha   a1 = -2.*cosw0   a2 = 1.-alpha
 * sin / cos of the float w0: argument reduction + polynomial in IEEE double, rounded to float once -- the correctly rounded
 * float (a libm's sinf / cosf, which is what the reference's std::sin(float) is, stays within 1 ULP of that; glibc's agrees
 * on 98.7 % of the arguments); |w0| >= 2^20 gives NaN coefficients.  raw6 [6][n_streams] receives a0 a1 a2 b0 b1 b2 (may be NULL);
 * df1 [5][n_streams] receives the rows a Flowz DF1 stage with fz_stream_param coefficients reads,
 * b0/a0 b1/a0 b2/a0 -a1/a0 -a2/a0 in float (may be NULL): pass a pointer into the `params` buffer. */
int fz_rbj_lowpass(const float* freq_dev, const float* q_dev, float sample_rate, uint64_t n_streams,
                   float* raw6_dev, float* df1_dev, void* hip_stream);
/* plain float4 copy kernel: the measured-copy-bandwidth yardstick of the roofline report      */
int fz_copy_probe(const float* src_dev, float* dst_dev, uint64_t n_floats, void* hip_stream);
/* Layout adapter for callers that hold one contiguous buffer per stream, as every closure of the
 * reference does (the sample loop of test/benchmark.cpp:137-147):
 *   stream-major  [n_streams][n_samples][n_wires]   <->   frames [n_samples][n_streams][n_wires]
 * (frames stream-tiled as fz_run_block_tiled takes them when tile_streams != 0: a multiple of 64 that
 * divides n_streams).  to_stream_major == 0: src is stream-major, dst are frames; != 0: the reverse.
 * One pass through LDS patches, reads and writes in 4 KiB runs; n_wires <= 64.                       */
int fz_transpose_frames(const float* src_dev, float* dst_dev, uint64_t n_streams, uint32_t n_samples, uint32_t n_wires,
                        uint32_t tile_streams, int to_stream_major, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWZ_HIP_H */
