// The published splitmix64 mixer: counter-based draws (a draw is the mix of a key built from a seed and the draw's indices), so
// results do not depend on scheduling.  Shared by pnp.hip (sample indices) and depth_aug.hip (per-pixel jitter).
#ifndef PP_SPLITMIX_H
#define PP_SPLITMIX_H

__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#endif
