// Micro-benchmark (diagnostic): does one tile of F = A - B P through the matrix pipe (tile_xty_blocks with the sweep's
// k-block mask, as lq_feedback_instance_mfma_pw forms it) carry the bits of the vector unit's fma(-b, p, a), or of
// a - b * p with two roundings, when every row of B holds at most one non-zero?  Random finite data, both precisions;
// prints the number of entries that differ per form.  hipcc --offload-arch=gfx950 -O3 -I ilqgames_amd/csrc -I include
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ilqg_mfma.hpp"

using namespace ilqg;

constexpr int kM = 6;  // rows of P (controls): k blocks kblock_mask<T>(0, kM)

// A, P, B: 16 x 16 column-major tiles (B: row = state, column = control).  out: [3][256] per tile.
template <typename T>
__global__ void k(const T* A, const T* P, const T* B, T* out) {
  using TL = Tile<T>;
  const int l = threadIdx.x, g = l >> 4, j = l & 15;
  const size_t tile = size_t(blockIdx.x) * 256;
  A += tile; P += tile; B += tile; out += 3 * tile;
  typename TL::vec nbt, pd, ad;
  for (int r = 0; r < 4; r++) {
    const int row = TL::row(g, r);
    nbt[r] = -B[j + 16 * row];  // D layout of -B^T
    pd[r] = P[row + 16 * j];
    ad[r] = A[row + 16 * j];
  }
  const typename TL::vec f = tile_xty_blocks<T, kblock_mask<T>(0, kM)>(nbt, pd, ad);
  for (int r = 0; r < 4; r++) {
    const int row = TL::row(g, r);
    int c = 0;
    T b = T(0);
    for (int q = 0; q < kM; q++)
      if (B[row + 16 * q] != T(0)) { c = q; b = B[row + 16 * q]; }
    const T p = P[c + 16 * j], a = A[row + 16 * j];
    out[row + 16 * j] = f[r];
    out[256 + row + 16 * j] = __builtin_fma(-b, p, a);
    {
#pragma clang fp contract(off)
      const T bp = b * p;
      out[512 + row + 16 * j] = a - bp;
    }
  }
}

static unsigned long long s = 0x9e3779b97f4a7c15ull;
static double rnd() {  // (-1, 1) times a power of two from a wide range
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  const double u = double(s >> 11) / double(1ull << 53) * 2.0 - 1.0;
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return u * double(1ull << ((s >> 40) % 12));
}

template <typename T>
static void run(const char* name) {
  const int tiles = 512;
  std::vector<T> A(256 * tiles), P(256 * tiles), B(256 * tiles, T(0)), out(3 * 256 * tiles);
  for (auto& v : A) v = T(rnd());
  for (auto& v : P) v = T(rnd());
  for (int t = 0; t < tiles; t++) {
    // one entry per column of B, in distinct rows; even tiles: the headline's rows and dt, odd tiles: random ones
    const int head[kM] = {3, 4, 8, 9, 12, 13};
    bool used[16] = {};
    for (int q = 0; q < kM; q++) {
      int row = head[q];
      if (t & 1) do { row = int((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33) % 15; } while (used[row]);
      used[row] = true;
      B[size_t(t) * 256 + row + 16 * q] = (t & 1) ? T(rnd()) : T(0.1);
    }
  }
  T *dA, *dP, *dB, *dO;
  const size_t bytes = A.size() * sizeof(T);
  hipMalloc(&dA, bytes); hipMalloc(&dP, bytes); hipMalloc(&dB, bytes); hipMalloc(&dO, 3 * bytes);
  hipMemcpy(dA, A.data(), bytes, hipMemcpyHostToDevice);
  hipMemcpy(dP, P.data(), bytes, hipMemcpyHostToDevice);
  hipMemcpy(dB, B.data(), bytes, hipMemcpyHostToDevice);
  k<T><<<tiles, 64>>>(dA, dP, dB, dO);
  if (hipMemcpy(out.data(), dO, 3 * bytes, hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: HIP error\n", name); exit(1); }
  long long d_fma = 0, d_two = 0, two_vs_fma = 0, n = 0;
  for (int t = 0; t < tiles; t++)
    for (int e = 0; e < 256; e++) {
      if (e % 16 == 15 || e / 16 == 15) continue;
      const T m = out[size_t(t) * 768 + e], f = out[size_t(t) * 768 + 256 + e], w = out[size_t(t) * 768 + 512 + e];
      n++;
      d_fma += std::memcmp(&m, &f, sizeof(T)) != 0 && !(m == f);
      d_two += !(m == w);
      two_vs_fma += !(f == w);
    }
  printf("%s: %lld entries; matrix pipe != fma(-b, p, a): %lld; matrix pipe != a - b * p (two roundings): %lld; "
         "(the two vector forms differ in %lld)\n", name, n, d_fma, d_two, two_vs_fma);
}

int main() {
  run<double>("f64");
  run<float>("f32");
  return 0;
}
