// The kernarg image of a launch, built in one place (no HIP in here: the layout compiles and is tested on its own,
// tests/cpp/kernargs_layout.cpp).  Every kernel's argument struct is
//   [header][the window of a stream-major launch: rows_total, row0][max(n, 1) floats][padding to 8 bytes][max(m, 1) doubles]
// -- the header is the launch site's struct (its static_assert holds it to the kernel's), the floats are the uniform coefficient slots,
// the doubles the float64 literals of the frame kernels (the other kernels have no such tail).  A buffer of another size does not
// launch the kernel, and a pointer at another offset faults the card.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>

namespace fz {

// the window of a stream-major launch: rows [row0, row0 + n_samples) of buffers [n_streams][rows_total][wire]
struct SmWindow {
   uint32_t rows_total, row0;
};
static_assert(sizeof(SmWindow) == 2 * sizeof(unsigned int), "SmWindow is the kernels' rows_total and row0");

class KernArgs {
public:
   static constexpr size_t kInlineBytes = 1024;             // images up to this size live in the object: no allocation on the launch path

   // n_f64: the count of the float64 tail; none: the kernel's struct ends behind the floats
   KernArgs(size_t header_bytes, bool window, size_t n_f32, std::optional<size_t> n_f64 = std::nullopt)
      : header_bytes_(header_bytes), off_f32_(header_bytes + (window ? sizeof(SmWindow) : 0)), n_f32_(n_f32),
        off_f64_((off_f32_ + sizeof(float) * std::max<size_t>(n_f32, 1) + 7) & ~size_t(7)), n_f64_(n_f64.value_or(0)),
        size_(n_f64 ? off_f64_ + sizeof(double) * std::max<size_t>(*n_f64, 1) : off_f64_)
   {
      if (size_ > kInlineBytes) big_.reset(new char[size_]);
      buf_ = big_ ? big_.get() : small_;
      std::memset(buf_, 0, size_);
   }
   KernArgs(const KernArgs&) = delete;
   KernArgs& operator=(const KernArgs&) = delete;

   // the first header_bytes of `header` (again and again: the tails stay)
   void set_header(const void* header) { std::memcpy(buf_, header, header_bytes_); }
   void set_window(const SmWindow& w) { std::memcpy(buf_ + header_bytes_, &w, sizeof w); }
   // the coefficient tails, as many as the image was made for (the caller holds the lock that guards them)
   void copy_tails(const float* f32, const double* f64 = nullptr)
   {
      if (n_f32_) std::memcpy(buf_ + off_f32_, f32, sizeof(float) * n_f32_);
      if (n_f64_) std::memcpy(buf_ + off_f64_, f64, sizeof(double) * n_f64_);
   }
   char* data() { return buf_; }
   const char* data() const { return buf_; }
   size_t size() const { return size_; }
   bool is_inline() const { return !big_; }

private:
   size_t header_bytes_, off_f32_, n_f32_, off_f64_, n_f64_, size_;
   alignas(8) char small_[kInlineBytes];
   std::unique_ptr<char[]> big_;
   char* buf_;
};

}  // namespace fz
