// Host-only checks of the graph functions in the C++ front end (no GPU): flowz::abs / sqrt / exp / tanh / min / max build the IR
// nodes of include/flowz_hip.h with the types C++ gives them, keep the arities, and refuse what C++ refuses.
#include <complex>
#include <cstdio>
#include <vector>

#include <flowz/flowz.hpp>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// kinds and dtypes of the lowered IR of e (fz_compile), or rc < 0
static std::vector<fz_ir_node> ir_of(const fz_expr* e, int* rc)
{
   fz_program* p = nullptr;
   *rc = fz_compile(e, &p);
   if (*rc < 0) return {};
   std::vector<fz_ir_node> v((size_t)fz_program_ir(p, nullptr, 0));
   fz_program_ir(p, v.data(), (uint32_t)v.size());
   fz_program_destroy(p);
   return v;
}

static int count(const std::vector<fz_ir_node>& v, uint32_t kind, int dtype = -1)
{
   int n = 0;
   for (const fz_ir_node& x : v) n += x.kind == kind && (dtype < 0 || (int)x.dtype == dtype);
   return n;
}

int main()
{
   using namespace flowz;
   int rc = 0;

   // a one-node function keeps the operand's input arity and gives one output wire
   auto t = flowz::tanh(_2);
   static_assert(decltype(t)::ins == 2 && decltype(t)::outs == 1, "");
   auto m = flowz::min(_1, _3[_2]);
   static_assert(decltype(m)::ins == 3 && decltype(m)::outs == 1, "");
   auto ms = flowz::max(0.25f, _1);
   static_assert(decltype(ms)::ins == 1 && decltype(ms)::outs == 1, "");

   // float wires: float nodes
   auto f = flowz::tanh(_1) + flowz::exp(_1) + flowz::sqrt(flowz::abs(_1)) + flowz::min(flowz::max(_1, -0.5f), 0.5f);
   auto v = ir_of(f.h.get(), &rc);
   CHECK(rc == 0);
   CHECK(count(v, FZ_IR_TANH, 0) == 1 && count(v, FZ_IR_EXP, 0) == 1 && count(v, FZ_IR_SQRT, 0) == 1 && count(v, FZ_IR_ABS, 0) == 1);
   CHECK(count(v, FZ_IR_MIN, 0) == 1 && count(v, FZ_IR_MAX, 0) == 1);

   // a double scalar stays double: tanh(0.5 * _1) is a double tanh; min(_1, 0.25) a double min of the widened wire
   auto d = flowz::tanh(0.5 * _1) + flowz::min(_1, 0.25);
   v = ir_of(d.h.get(), &rc);
   CHECK(rc == 0);
   CHECK(count(v, FZ_IR_TANH, 1) == 1 && count(v, FZ_IR_MIN, 1) == 1 && count(v, FZ_IR_TANH, 0) == 0);

   // the same function of the same wire is one node (sharing)
   auto sh = flowz::exp(_1) * flowz::exp(_1);
   v = ir_of(sh.h.get(), &rc);
   CHECK(rc == 0 && count(v, FZ_IR_EXP) == 1);

   // functions inside a feedback loop: a saturating one-pole
   auto sat = ~(flowz::tanh(0.9f * _1[_1] + _2));
   static_assert(decltype(sat)::ins == 1 && decltype(sat)::outs == 1, "");
   auto prog = compile(sat);
   CHECK(prog.info().n_ops == 3 && prog.info().n_state == 1);

   // std::complex operands: min / max are no C++ operators (FZ_E_GRAPH), the others valid C++ but not built (FZ_E_UNSUPPORTED)
   const std::complex<float> c(0.5f, 0.25f);
   auto cm = flowz::min(c * _1, _1);
   v = ir_of(cm.h.get(), &rc);
   CHECK(rc == FZ_E_GRAPH);
   auto ct = flowz::tanh(c * _1);
   v = ir_of(ct.h.get(), &rc);
   CHECK(rc == FZ_E_UNSUPPORTED);

   // a multi-wire operand is refused by the C ABI as well (the template refuses it at compile time)
   fz_expr* two = fz_channel(_1.h.get(), _1.h.get());
   CHECK(fz_arith(FZ_OP_EXP, two, nullptr) == nullptr);
   fz_expr_release(two);

   if (failures) {
      std::printf("%d graph-function host checks FAILED\n", failures);
      return 1;
   }
   std::printf("all graph-function host checks passed\n");
   return 0;
}
