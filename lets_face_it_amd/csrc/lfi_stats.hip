// Per-array statistics of many fp32 arrays in one pass (lfi_segment_stats): which tensors, inputs and frames hold a NaN or an Inf,
// and the 2-norm of the finite part of each. Also the same work behind the non-finite step guard (lfi_segment_stats_guard): the
// blame record of a skipped step, filled on the device in the step that decided to skip.
#include "lfi_common.h"

// Three launches, whatever the number of arrays:
//   plan    one workgroup: chunk prefix of the arrays (an array of len floats is ceil(len / SS_CH) chunks) into the work buffer;
//   chunks  one workgroup per chunk: fp64 sum of squares of the finite elements, NaN / Inf counts and the first non-finite index of
//           that chunk, as four 8-byte slots of the work buffer. No atomics: every slot has one writer;
//   finish  one workgroup, one thread per array: the chunk partials summed in chunk order, the record written, and - guarded form -
//           the blame header as the last act.
// The same three kernels serve both entry points (guard pointers null = unconditional), so the bits of a record are the same from
// either. A segment table that breaks its contract (a range outside [0, n), overlaps that push the chunk total past the host's
// bound) costs correctness of the numbers only: such ranges count as empty, the prefix is clamped to the grid.
namespace {
constexpr int SS_CH = 4096;            // floats per chunk: 256 threads x 4 x 16 bytes
constexpr int SS_MAX_EXTRA = 8;
constexpr unsigned long long SS_NONE = ~0ull;

struct StatArrays {
  const float* flat;                   // the flat buffer the segment table indexes
  long n;                              // its length in floats
  const long* segs;                    // nseg (offset, length) pairs, on the device
  int nseg, nextra;
  const float* xp[SS_MAX_EXTRA];
  long xn[SS_MAX_EXTRA];
};

// array a of the call: its first element and its length (a range outside the flat buffer is empty)
__device__ __forceinline__ long stat_array(const StatArrays& sa, int a, const float** base) {
  if (a < sa.nseg) {
    const long off = sa.segs[2 * a], len = sa.segs[2 * a + 1];
    const bool ok = off >= 0 && len >= 0 && off <= sa.n && len <= sa.n - off;
    *base = sa.flat + (ok ? off : 0);
    return ok ? len : 0;
  }
  // (a chain of selects, not an index: a runtime index into a by-value argument array would go through scratch)
  const int x = a - sa.nseg;
  const float* p = sa.xp[0];
  long len = sa.xn[0];
#pragma unroll
  for (int i = 1; i < SS_MAX_EXTRA; ++i) {
    if (x == i) {
      p = sa.xp[i];
      len = sa.xn[i];
    }
  }
  *base = p;
  return len;
}

__device__ __forceinline__ bool stat_skip(const unsigned long long* rec, const unsigned long long* blame) {
  return rec != nullptr && (rec[LFI_GUARD_APPLY] != 0 || blame[LFI_BLAME_FILLED] != 0);
}

// prefix[a] = first chunk of array a, prefix[narr] = their number, each clamped to the grid of the chunks launch
__global__ __launch_bounds__(256) void stat_plan_kernel(StatArrays sa, long* __restrict__ prefix, long max_chunks,
                                                        const unsigned long long* __restrict__ rec,
                                                        const unsigned long long* __restrict__ blame) {
  if (stat_skip(rec, blame)) return;
  __shared__ long tot[256];
  const int narr = sa.nseg + sa.nextra;
  const int per = (narr + 255) / 256;
  const int a0 = min(narr, (int)threadIdx.x * per), a1 = min(narr, a0 + per);
  long mine = 0;
  for (int a = a0; a < a1; ++a) {
    const float* base;
    mine += (stat_array(sa, a, &base) + SS_CH - 1) / SS_CH;
  }
  tot[threadIdx.x] = mine;
  __syncthreads();
  long before = 0;      // (256 adds from LDS per thread: the launch is latency, not work)
  for (int t = 0; t < (int)threadIdx.x; ++t) before += tot[t];
  for (int a = a0; a < a1; ++a) {
    const float* base;
    prefix[a] = min(before, max_chunks);
    before += (stat_array(sa, a, &base) + SS_CH - 1) / SS_CH;
  }
  if (threadIdx.x == 255) prefix[narr] = min(before, max_chunks);
}

struct ChunkAcc {
  double s;
  int nan, inf, first;      // first: index inside the chunk, SS_CH = none
};

__device__ __forceinline__ void stat_take(ChunkAcc& acc, float x, int idx) {
  const unsigned b = __float_as_uint(x);
  if ((b & 0x7f800000u) == 0x7f800000u) {
    if (b & 0x007fffffu) ++acc.nan;
    else ++acc.inf;
    acc.first = min(acc.first, idx);
  } else {
    acc.s += (double)x * (double)x;
  }
}

__global__ __launch_bounds__(256) void stat_chunk_kernel(StatArrays sa, const long* __restrict__ prefix,
                                                         unsigned long long* __restrict__ part,
                                                         const unsigned long long* __restrict__ rec,
                                                         const unsigned long long* __restrict__ blame) {
  if (stat_skip(rec, blame)) return;
  __shared__ double red_s[4];
  __shared__ int red_i[4][3];
  const int narr = sa.nseg + sa.nextra;
  const long b = blockIdx.x;
  if (b >= prefix[narr]) return;
  // the array whose chunks hold chunk b: the last a with prefix[a] <= b (uniform over the workgroup: scalar loads)
  int lo = 0, hi = narr - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const float* base;
  const long len = stat_array(sa, lo, &base);
  const long c0 = (b - prefix[lo]) * SS_CH;
  const int m = (int)min((long)SS_CH, len - c0);      // >= 1: chunk b exists
  const float* __restrict__ p = base + c0;
  // 16-byte loads over the aligned middle, scalar loads over the (at most three) floats before and after it
  const int head = min(m, (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2));
  const int n4 = (m - head) >> 2;
  const int tail0 = head + (n4 << 2);
  ChunkAcc acc = {0.0, 0, 0, SS_CH};
  const int t = threadIdx.x;
  if (t < head) stat_take(acc, p[t], t);
  const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
  float4 v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = t + 256 * u;
    v[u] = i < n4 ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = head + 4 * (t + 256 * u);
    if (t + 256 * u < n4) {
      stat_take(acc, v[u].x, i);
      stat_take(acc, v[u].y, i + 1);
      stat_take(acc, v[u].z, i + 2);
      stat_take(acc, v[u].w, i + 3);
    }
  }
  if (tail0 + t < m) stat_take(acc, p[tail0 + t], tail0 + t);
  // workgroup totals in a fixed order: the shuffle tree, then the four waves
  acc.s = wave_sum_d(acc.s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc.nan += __shfl_xor(acc.nan, o, 64);
    acc.inf += __shfl_xor(acc.inf, o, 64);
    acc.first = min(acc.first, __shfl_xor(acc.first, o, 64));
  }
  if ((t & 63) == 0) {
    red_s[t >> 6] = acc.s;
    red_i[t >> 6][0] = acc.nan;
    red_i[t >> 6][1] = acc.inf;
    red_i[t >> 6][2] = acc.first;
  }
  __syncthreads();
  if (t != 0) return;
  const double s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
  const int first = min(min(red_i[0][2], red_i[1][2]), min(red_i[2][2], red_i[3][2]));
  unsigned long long* o = part + (long)LFI_SEG_SLOTS * b;
  o[LFI_SEG_SUMSQ] = (unsigned long long)__double_as_longlong(s);
  o[LFI_SEG_NAN] = (unsigned long long)(red_i[0][0] + red_i[1][0] + red_i[2][0] + red_i[3][0]);
  o[LFI_SEG_INF] = (unsigned long long)(red_i[0][1] + red_i[1][1] + red_i[2][1] + red_i[3][1]);
  o[LFI_SEG_FIRST] = first < SS_CH ? (unsigned long long)(c0 + first) : SS_NONE;
}

__global__ __launch_bounds__(256) void stat_finish_kernel(int narr, const long* __restrict__ prefix,
                                                          const unsigned long long* __restrict__ part,
                                                          unsigned long long* __restrict__ out,
                                                          const unsigned long long* __restrict__ rec, unsigned long long* blame) {
  if (stat_skip(rec, blame)) return;
  for (int a = threadIdx.x; a < narr; a += 256) {
    const long c0 = prefix[a], c1 = prefix[a + 1];
    double s = 0.0;
    unsigned long long nan = 0, inf = 0, first = SS_NONE;
    for (long c = c0; c < c1; c += 8) {      // eight partials asked for at once, added in chunk order (+0.0 behind the last one)
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = c + u < c1 ? __longlong_as_double((long long)part[LFI_SEG_SLOTS * (c + u) + LFI_SEG_SUMSQ]) : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s += v[u];
        if (c + u < c1) {
          const unsigned long long* q = part + LFI_SEG_SLOTS * (c + u);
          nan += q[LFI_SEG_NAN];
          inf += q[LFI_SEG_INF];
          first = min(first, q[LFI_SEG_FIRST]);      // (chunk partials carry indices within the array)
        }
      }
    }
    unsigned long long* o = out + (long)LFI_SEG_SLOTS * a;
    o[LFI_SEG_SUMSQ] = (unsigned long long)__double_as_longlong(s);
    o[LFI_SEG_NAN] = nan;
    o[LFI_SEG_INF] = inf;
    o[LFI_SEG_FIRST] = first;
  }
  if (rec == nullptr) return;
  // the table first, then the step it belongs to, then the flag that says so: nothing of this call is behind this store
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  blame[LFI_BLAME_STEP] = rec[LFI_GUARD_APPLIED] + rec[LFI_GUARD_SKIPPED];
  __threadfence();
  blame[LFI_BLAME_FILLED] = 1ull;
}

// chunks the host can promise the device will not exceed: disjoint segments inside [0, n) make at most n / CH + nseg of them
long stat_max_chunks(long n, int nseg, int nextra, const long* xlen) {
  long c = nseg > 0 ? (n + SS_CH - 1) / SS_CH + nseg : 0;
  for (int i = 0; i < nextra; ++i) c += (xlen[i] + SS_CH - 1) / SS_CH;
  return c;
}

int stat_launch(const char* who, const float* flat, long n, const long* segs, int nseg, int nextra, const float* const* xptrs,
                const long* xlen, void* out, void* work, const void* rec, void* blame, bool guarded, void* stream) {
  LFI_REQUIRE(nseg >= 0, "%s: nseg = %d", who, nseg);
  LFI_REQUIRE(nextra >= 0 && nextra <= SS_MAX_EXTRA, "%s: %d extra arrays (at most %d)", who, nextra, SS_MAX_EXTRA);
  LFI_REQUIRE(n >= 0, "%s: n = %ld", who, n);
  LFI_REQUIRE(nseg == 0 || (flat && segs), "%s: null flat buffer / segment table", who);
  LFI_REQUIRE(nseg == 0 || (reinterpret_cast<uintptr_t>(segs) & 7) == 0, "%s: misaligned segment table", who);
  LFI_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 3) == 0, "%s: misaligned flat buffer", who);
  LFI_REQUIRE(nextra == 0 || (xptrs && xlen), "%s: null extra-array lists", who);
  StatArrays sa = {};
  for (int i = 0; i < nextra; ++i) {
    LFI_REQUIRE(xlen[i] >= 0, "%s: extra array %d: length %ld", who, i, xlen[i]);
    LFI_REQUIRE(xlen[i] == 0 || xptrs[i], "%s: extra array %d: null pointer", who, i);
    LFI_REQUIRE((reinterpret_cast<uintptr_t>(xptrs[i]) & 3) == 0, "%s: extra array %d: misaligned", who, i);
    sa.xp[i] = xptrs[i];
    sa.xn[i] = xlen[i];
  }
  LFI_REQUIRE(work && (reinterpret_cast<uintptr_t>(work) & 7) == 0, "%s: null / misaligned work buffer", who);
  if (guarded) {
    LFI_REQUIRE(rec && (reinterpret_cast<uintptr_t>(rec) & 7) == 0, "%s: null / misaligned guard record", who);
    LFI_REQUIRE(blame && (reinterpret_cast<uintptr_t>(blame) & 7) == 0, "%s: null / misaligned blame record", who);
  } else {
    LFI_REQUIRE(out && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "%s: null / misaligned record", who);
  }
  const int narr = nseg + nextra;
  if (narr == 0 && !guarded) return LFI_OK;
  sa.flat = flat;
  sa.n = n;
  sa.segs = segs;
  sa.nseg = nseg;
  sa.nextra = nextra;
  const long max_chunks = stat_max_chunks(n, nseg, nextra, xlen);
  LFI_REQUIRE(max_chunks < (1L << 24), "%s: %ld chunks (one workgroup each; fewer than 2^24)", who, max_chunks);
  hipStream_t st = (hipStream_t)stream;
  long* prefix = reinterpret_cast<long*>(work);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(work) + narr + 1;
  const unsigned long long* r = reinterpret_cast<const unsigned long long*>(rec);
  unsigned long long* bl = reinterpret_cast<unsigned long long*>(blame);
  unsigned long long* table = guarded ? bl + LFI_BLAME_HEAD : reinterpret_cast<unsigned long long*>(out);
  hipLaunchKernelGGL(stat_plan_kernel, dim3(1), dim3(256), 0, st, sa, prefix, max_chunks, r, (const unsigned long long*)bl);
  LFI_LAUNCH_CHECK(who);
  if (max_chunks > 0) {
    hipLaunchKernelGGL(stat_chunk_kernel, dim3((unsigned)max_chunks), dim3(256), 0, st, sa, (const long*)prefix, part, r,
                       (const unsigned long long*)bl);
    LFI_LAUNCH_CHECK(who);
  }
  hipLaunchKernelGGL(stat_finish_kernel, dim3(1), dim3(256), 0, st, narr, (const long*)prefix, (const unsigned long long*)part, table, r,
                     bl);
  LFI_LAUNCH_CHECK(who);
  return LFI_OK;
}
}  // namespace

extern "C" long lfi_segment_stats_chunk(void) { return SS_CH; }

extern "C" long lfi_segment_stats_work_floats(long n, int nseg, int nextra, const long* xlen) {
  LFI_REQUIRE(n >= 0 && nseg >= 0 && nextra >= 0 && nextra <= SS_MAX_EXTRA && (nextra == 0 || xlen),
              "lfi_segment_stats_work_floats: bad arguments");
  for (int i = 0; i < nextra; ++i) LFI_REQUIRE(xlen[i] >= 0, "lfi_segment_stats_work_floats: extra array %d: length %ld", i, xlen[i]);
  // 8-byte slots: the chunk prefix (one per array and the total), then LFI_SEG_SLOTS per chunk
  return 2 * ((long)nseg + nextra + 1 + LFI_SEG_SLOTS * stat_max_chunks(n, nseg, nextra, xlen));
}

extern "C" int lfi_segment_stats(const float* flat, long n, const long* segs, int nseg, int nextra, const float* const* xptrs,
                                 const long* xlen, void* out, void* work, void* stream) {
  return stat_launch("lfi_segment_stats", flat, n, segs, nseg, nextra, xptrs, xlen, out, work, nullptr, nullptr, false, stream);
}

extern "C" int lfi_segment_stats_guard(const float* flat, long n, const long* segs, int nseg, int nextra, const float* const* xptrs,
                                       const long* xlen, const void* rec, void* blame, void* work, void* stream) {
  return stat_launch("lfi_segment_stats_guard", flat, n, segs, nseg, nextra, xptrs, xlen, nullptr, work, rec, blame, true, stream);
}
