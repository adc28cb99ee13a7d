// The sender's clue kernel and the recipient's clue opening (include/omr_gpu.h "Sender"). Included by
// keygen_gpu.hip alone, inside its anonymous namespace, after fill_words / pack_gaussians / CLUE_WORDS /
// CDT_LDS, which stay written once there.
#pragma once

// ------------------------------------------------------------------------------------------
// Clues under a table of keys: message m of the launch under key recipient[m] (NULL: key 0), from
// Stream(seed, DOM_CLUE, first + m) exactly as gen_clues_kernel draws it. One 64-thread workgroup per
// message. What differs from gen_clues_kernel is the key: it is fetched from table [n_keys][2][512] u16
// with one 16-byte load per lane and half (1 KiB of contiguous lanes each), issued before the stream is
// computed so that a miss in the table hides behind the ChaCha blocks. An id >= n_keys leaves the clue
// unwritten and records base + m in *err (the smallest wins). The stream expansion, the Gaussian walk,
// the product and the stores are gen_clues_kernel's, so the bits are.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sender_clues_kernel(const uint16_t *__restrict__ table, uint32_t n_keys,
                                                          const uint32_t *__restrict__ recipient,
                                                          const uint64_t *__restrict__ cdt, int cdt_n,
                                                          uint64_t seed, uint64_t first, size_t count, size_t base,
                                                          uint16_t *__restrict__ clue_a,
                                                          uint16_t *__restrict__ clue_b,
                                                          unsigned long long *__restrict__ err) {
  __shared__ uint32_t w[CLUE_WORDS];
  __shared__ int32_t A[N0], B[N0], es[N0 + CLUES];
  __shared__ uint64_t tab[CDT_LDS];
  const size_t m = blockIdx.x;
  const int tid = threadIdx.x;
  if (m >= count) return;
  const uint32_t id = recipient ? (uint32_t)__builtin_amdgcn_readfirstlane((int)recipient[m]) : 0u;
  if (id >= n_keys) {  // wave-uniform: the whole workgroup leaves before any barrier
    if (tid == 0) atomicMin(err, (unsigned long long)(base + m));
    return;
  }
  const uint4 *key = reinterpret_cast<const uint4 *>(table + (size_t)id * 2 * N0);
  const uint4 ka = key[tid], kb = key[N0 / 8 + tid];  // words [8 tid, 8 tid + 8) of a and of b
  for (int i = tid; i < cdt_n; i += 64) tab[i] = cdt[i];
  fill_words(w, CLUE_WORDS / 16, seed, DOM_CLUE, first + m);
  {
    const uint32_t a4[4] = {ka.x, ka.y, ka.z, ka.w}, b4[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      A[8 * tid + 2 * k] = (int32_t)(a4[k] & 0xffffu);
      A[8 * tid + 2 * k + 1] = (int32_t)(a4[k] >> 16);
      B[8 * tid + 2 * k] = (int32_t)(b4[k] & 0xffffu);
      B[8 * tid + 2 * k + 1] = (int32_t)(b4[k] >> 16);
    }
  }
  __syncthreads();
  pack_gaussians(w, CLUE_WORDS, 16, 3 * (N0 + CLUES), tab, cdt_n);
  if (tid == 0) {
    int p = 16;
    for (int i = 0; i < N0 + CLUES; ++i) {
      const int v = (int)w[p];
      es[i] = v >> 2;
      p += v & 3;
    }
  }
  __syncthreads();
  // r = words 0..15, bit b of word k is r[32k + b]
  int acc[N0 / 64];
#pragma unroll
  for (int j = 0; j < N0 / 64; ++j) acc[j] = es[tid + 64 * j];
  int accb = tid < CLUES ? es[N0 + tid] : 0;
  for (int k = 0; k < N0 / 32; ++k) {
    uint32_t bits = __builtin_amdgcn_readfirstlane(w[k]);
    while (bits) {
      const int t = 32 * k + __builtin_ctz(bits);
      bits &= bits - 1;
#pragma unroll
      for (int j = 0; j < N0 / 64; ++j) {
        const int d = tid + 64 * j - t;  // u[o] += A[o - t] (o >= t), -= A[o - t + 512]
        const int a = A[d & (N0 - 1)];
        acc[j] += d >= 0 ? a : -a;
      }
      if (tid < CLUES) {
        const int d = tid - t;
        const int b = B[d & (N0 - 1)];
        accb += d >= 0 ? b : -b;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < N0 / 64; ++j) clue_a[m * N0 + tid + 64 * j] = (uint16_t)(acc[j] & (Q0 - 1));
  if (tid < CLUES) clue_b[m * CLUES + tid] = (uint16_t)(accb & (Q0 - 1));
}

// ------------------------------------------------------------------------------------------
// Clue opening: a wave opens OPEN_PER_WAVE consecutive messages, OPEN_WAVES waves per workgroup. The
// seven phases b_i - (a * s0)[i] (negacyclic, i < 7) over ONE read of a message's 1 KiB mask: lane l loads
// words [8 l, 8 l + 8) with one 16-byte load (the wave reads each kilobyte contiguously), and all of the
// wave's messages are loaded before the first is opened, so that 4 KiB per wave are in flight. Word
// k = 8 l + j meets s0[(i - k) mod 512] with the sign of the wrap (minus when k > i). For one lane those
// are the 14 consecutive bits of s0 from (-8 l - 7) mod 512 on; bit 7 - j + i of that window belongs to
// (j, i). s0 arrives as 16 words in the kernel arguments (the call hands it over itself, no allocation)
// and is put in LDS, where a lane-dependent word index costs nothing. The seven sums are reduced over the
// wave with xor shuffles; lanes 0..6 then finish clue i = lane.
// ------------------------------------------------------------------------------------------
constexpr int OPEN_WAVES = 4, OPEN_PER_WAVE = 4;
struct S0Bits {
  uint32_t w[N0 / 32];  // bit b of word k is s0[32 k + b]
};

__global__ __launch_bounds__(64 * OPEN_WAVES) void clue_open_kernel(S0Bits s0, const uint16_t *__restrict__ clue_a,
                                                                    const uint16_t *__restrict__ clue_b, size_t count,
                                                                    uint8_t *__restrict__ values,
                                                                    uint8_t *__restrict__ pertinent,
                                                                    uint8_t *__restrict__ max_abs_noise) {
  __shared__ uint32_t sw[N0 / 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < N0 / 32) sw[threadIdx.x] = s0.w[threadIdx.x];
  __syncthreads();
  const size_t m0 = ((size_t)blockIdx.x * OPEN_WAVES + wave) * OPEN_PER_WAVE;
  if (m0 >= count) return;  // wave-uniform, after the only barrier
  uint4 q[OPEN_PER_WAVE];
  int body[OPEN_PER_WAVE];
#pragma unroll
  for (int p = 0; p < OPEN_PER_WAVE; ++p) {
    const bool in = m0 + p < count;  // wave-uniform
    q[p] = in ? reinterpret_cast<const uint4 *>(clue_a + (m0 + p) * N0)[lane] : make_uint4(0, 0, 0, 0);
    body[p] = in && lane < CLUES ? clue_b[(m0 + p) * CLUES + lane] & (Q0 - 1) : 0;
  }
  const int base = (N0 - 8 * lane - 7) & (N0 - 1);
  const uint32_t lo = sw[base >> 5], hi = sw[((base >> 5) + 1) & (N0 / 32 - 1)];
  const uint32_t win = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (base & 31)) & 0x3fffu;
#pragma unroll
  for (int p = 0; p < OPEN_PER_WAVE; ++p) {
    const size_t m = m0 + p;
    if (m >= count) break;
    const uint32_t q4[4] = {q[p].x, q[p].y, q[p].z, q[p].w};
    int sum[CLUES];
#pragma unroll
    for (int i = 0; i < CLUES; ++i) sum[i] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int u = (int)((q4[j >> 1] >> (16 * (j & 1))) & (uint32_t)(Q0 - 1));
      const int k = 8 * lane + j;
#pragma unroll
      for (int i = 0; i < CLUES; ++i) {
        const int t = ((win >> (7 - j + i)) & 1u) ? u : 0;
        sum[i] += k > i ? -t : t;
      }
    }
#pragma unroll
    for (int i = 0; i < CLUES; ++i)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) sum[i] += __shfl_xor(sum[i], d, 64);
    int mine = 0;  // the sum of clue i = lane
#pragma unroll
    for (int i = 0; i < CLUES; ++i) mine = lane == i ? sum[i] : mine;
    int value = 0, noise = 0;
    if (lane < CLUES) {
      const int phase = (body[p] - mine) & (Q0 - 1);
      value = ((8 * phase + Q0 / 2) >> 11) & 7;
      noise = ((phase - 256 * value + Q0 / 2) & (Q0 - 1)) - Q0 / 2;  // [-128, 127]
      noise = noise < 0 ? -noise : noise;
      if (values) values[m * CLUES + lane] = (uint8_t)value;
    }
    const unsigned long long any = __ballot(value != 0);
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) noise = max(noise, __shfl_xor(noise, d, 64));  // lanes 0..7; lane 7 holds 0
    if (lane == 0) {
      if (pertinent) pertinent[m] = (uint8_t)(any == 0);
      if (max_abs_noise) max_abs_noise[m] = (uint8_t)noise;
    }
  }
}
