// Packed strict upper triangle of an n x n matrix (the bpp matrices), 0-based
// i < j: host code and the fold kernels.
#pragma once

#include <cstddef>

namespace sk {

#if defined(__HIP__)
__host__ __device__
#endif
inline size_t tri_index(int n, int i, int j) {
  return (size_t)i * n - (size_t)i * (i + 1) / 2 + (size_t)(j - i - 1);
}

}  // namespace sk
