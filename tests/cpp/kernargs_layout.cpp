// The kernarg image KernArgs builds (zignal_amd/csrc/fz_kernargs.hpp) against the layout of the kernels' argument structs, written
// out here byte by byte: [header][rows_total, row0 of a stream-major launch][max(n, 1) floats][pad to 8][max(m, 1) doubles where the
// kernel has a float64 tail].  Host code only: built with -fsanitize=address,undefined by tests/test_kernargs_host.py.
#include <cstdio>
#include <cstring>
#include <optional>
#include <vector>

#include "fz_kernargs.hpp"

using fz::KernArgs;
using fz::SmWindow;

// the header structs of the launch sites, as their static_asserts state them
static const struct {
   const char* name;
   size_t bytes;
} kHeaders[] = {
   {"ArgsHeader (fz_args)", 6 * 8 + 8 + 10 * 4},
   {"PcmArgsHeader (fz_pcm_args)", 4 * 8 + 8 + 2 * 4},
   {"PcmSmArgsHeader (fz_pcm_sm_args)", 4 * 8 + 8 + 4 * 4},
   {"AdjArgsHeader (fz_adj_args)", 10 * 8 + 8 + 2 * 4},
   {"kAdjLossHeaderBytes (fz_adj_args under FZ_LOSS)", 12 * 8 + 8 + 2 * 4 + 4},   // an odd multiple of 4
   {"StatesArgsHeader (fz_states_args)", 5 * 8 + 8 + 2 * 4},
};

static int failures = 0;

static void expect(bool ok, const char* what, const char* header, bool window, size_t n, int m)
{
   if (ok) return;
   ++failures;
   std::printf("FAIL %s: %s, window %d, %zu floats, %d doubles\n", what, header, (int)window, n, m);
}

int main()
{
   int cases = 0;
   for (const auto& hd : kHeaders)
      for (bool window : {false, true})
         for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(3), size_t(300)})
            for (int m : {-1, 0, 3}) {                       // -1: the kernel's struct has no float64 tail
               std::vector<unsigned char> header(hd.bytes + 8), header2(hd.bytes + 8);   // (longer than the header: only its bytes may be taken)
               for (size_t i = 0; i < header.size(); ++i) header[i] = (unsigned char)(1 + i * 7), header2[i] = (unsigned char)(3 + i * 11);
               std::vector<float> f32(n);
               for (size_t i = 0; i < n; ++i) f32[i] = 0.5f + (float)i;
               std::vector<double> f64(m > 0 ? m : 0);
               for (size_t i = 0; i < f64.size(); ++i) f64[i] = -1.25 - (double)i;
               const SmWindow w{0x11223344u, 0x55667788u};

               // the expected image, from the kernel structs
               const size_t off_window = hd.bytes;
               const size_t off_f32 = hd.bytes + (window ? 8 : 0);
               const size_t off_f64 = (off_f32 + 4 * (n ? n : 1) + 7) / 8 * 8;
               const size_t size = m < 0 ? off_f64 : off_f64 + 8 * (size_t)(m ? m : 1);
               std::vector<unsigned char> want(size, 0);
               std::memcpy(want.data(), header.data(), hd.bytes);
               if (window) {
                  std::memcpy(want.data() + off_window, &w.rows_total, 4);
                  std::memcpy(want.data() + off_window + 4, &w.row0, 4);
               }
               if (n) std::memcpy(want.data() + off_f32, f32.data(), 4 * n);
               if (m > 0) std::memcpy(want.data() + off_f64, f64.data(), 8 * (size_t)m);

               KernArgs ka(hd.bytes, window, n, m < 0 ? std::nullopt : std::optional<size_t>((size_t)m));
               expect(ka.size() == size, "size", hd.name, window, n, m);
               expect(ka.is_inline() == (size <= 1024), "inline up to 1024 bytes", hd.name, window, n, m);
               if (ka.size() != size) continue;
               std::vector<unsigned char> zeros(size, 0);
               expect(std::memcmp(ka.data(), zeros.data(), size) == 0, "zero-filled", hd.name, window, n, m);
               ka.set_header(header.data());
               if (window) ka.set_window(w);
               ka.copy_tails(f32.data(), f64.data());
               expect(std::memcmp(ka.data(), want.data(), size) == 0, "image", hd.name, window, n, m);
               // the header again (the frame kernel's laps): the window and the tails stay
               ka.set_header(header2.data());
               std::memcpy(want.data(), header2.data(), hd.bytes);
               expect(std::memcmp(ka.data(), want.data(), size) == 0, "image after the header was rewritten", hd.name, window, n, m);
               ++cases;
            }
   std::printf("kernarg images: %d cases, %d failures\n", cases, failures);
   return failures ? 1 : 0;
}
