// Host-side check of the seven chunk window entry points' argument handling (lfi_stream.hip: stream_chunk_args), for a sanitizer
// build: every bad-argument case must return -1 with its own function's message before any launch, so no device is needed.
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//       tools/stream_chunk_args_check.cpp lets_face_it_amd/csrc/lfi_stream.hip lets_face_it_amd/csrc/lfi_core.hip -o stream_chunk_args_check
//   ./stream_chunk_args_check        (prints the number of cases, exit status 0; a miss names the case, exit status 1)
#include <cstdio>
#include <cstring>

#include "lfi.h"

static int g_cases = 0, g_missed = 0;

static void expect(int rc, const char* who, const char* what, const char* label) {
  ++g_cases;
  const char* msg = lfi_last_error();
  if (rc == -1 && std::strstr(msg, who) == msg && msg[std::strlen(who)] == ':' && std::strstr(msg, what)) return;
  ++g_missed;
  std::printf("MISS %s / %s: rc %d, message \"%s\" (wanted \"%s ... %s\")\n", who, label, rc, msg, who, what);
}

int main() {
  // fake device addresses: never dereferenced on the host, and no case here reaches a launch
  float* const dev = reinterpret_cast<float*>(0x4000);
  float* wins[2] = {dev, dev};
  float* seqs[2] = {dev, dev};
  const float* srcs[2] = {dev, dev};
  const float* no_first[2] = {nullptr, dev};
  const float* no_second[2] = {dev, nullptr};
  float* no_win[2] = {dev, nullptr};
  const int hist[2] = {3, 4}, dim[2] = {5, 6}, lead[2] = {0, 1}, deep[2] = {3, 6};
  const int* lens = reinterpret_cast<const int*>(dev);
  const int* roles = lens;
  unsigned* guard = nullptr;
  const int B = 2, n = 3, start = 4, k = 2, gen = 1, C = 6;
  const long ld = 3 * 6;

#define IN(...) lfi_stream_chunk_in(__VA_ARGS__, guard, nullptr)
#define IN_ROWS(...) lfi_stream_chunk_in_rows(__VA_ARGS__, guard, lens, nullptr)
#define GEN_IN(...) lfi_stream_chunk_gen_in(__VA_ARGS__, gen, dev, C, guard, nullptr)
#define ROLES_IN(...) lfi_stream_chunk_roles_in(__VA_ARGS__, gen, dev, C, roles, guard, nullptr)
#define OUT(...) lfi_stream_chunk_out(__VA_ARGS__, nullptr, nullptr)
#define OUT_ROWS(...) lfi_stream_chunk_out_rows(__VA_ARGS__, nullptr, lens, nullptr)
#define GEN_OUT(...) lfi_stream_chunk_gen_out(__VA_ARGS__, gen, dev, ld, nullptr, guard, nullptr)
  // what all seven share: the window tables, the window count, hist against start
#define SHARED(CALL_IN, CALL_OUT, in_name, out_name)                                                                              \
  expect(CALL_IN(B, n, start, k, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), in_name, "null pointer (window table)", "null tables"); \
  expect(CALL_IN(B, n, start, k, no_win, srcs, seqs, hist, dim, lead), in_name, "null pointer (window 1)", "null window");         \
  expect(CALL_IN(B, n, start, 9, wins, srcs, seqs, hist, dim, lead), in_name, "9 windows (1 .. 8)", "count 9");                    \
  expect(CALL_IN(B, n, start, k, wins, srcs, seqs, deep, dim, lead), in_name, "window 1: hist 6", "hist > start");                 \
  expect(CALL_IN(0, n, start, k, wins, srcs, seqs, hist, dim, lead), in_name, "batch 0", "no batch");                              \
  expect(CALL_IN(B, 0, start, k, wins, srcs, seqs, hist, dim, lead), in_name, "0 frames from frame 4", "no frames");               \
  expect(CALL_IN(B, n, start, k, wins, nullptr, seqs, hist, dim, lead), in_name, "null pointer (source table", "null source table"); \
  expect(CALL_IN(B, n, start, k, wins, no_first, seqs, hist, dim, lead), in_name, "null pointer (source 0)", "null source 0");     \
  if (out_name) {                                                                                                                  \
    expect(CALL_OUT(B, n, start, k, nullptr, nullptr, nullptr, nullptr, nullptr), out_name, "null pointer (window table)", "null tables"); \
    expect(CALL_OUT(B, n, start, k, wins, no_win, hist, dim, lead), out_name, "null pointer (window 1)", "null sequence"); \
    expect(CALL_OUT(B, n, start, 9, wins, seqs, hist, dim, lead), out_name, "9 windows (1 .. 8)", "count 9");                      \
    expect(CALL_OUT(B, n, start, k, wins, seqs, deep, dim, lead), out_name, "window 1: hist 6", "hist > start");                   \
  }
  SHARED(IN, OUT, "lfi_stream_chunk_in", "lfi_stream_chunk_out")
  SHARED(IN_ROWS, OUT_ROWS, "lfi_stream_chunk_in_rows", "lfi_stream_chunk_out_rows")
  SHARED(GEN_IN, GEN_OUT, "lfi_stream_chunk_gen_in", "lfi_stream_chunk_gen_out")
  SHARED(ROLES_IN, GEN_OUT, "lfi_stream_chunk_roles_in", static_cast<const char*>(nullptr))

  // the generated window's source: required by every variant but gen_in
  expect(IN(B, n, start, k, wins, no_second, seqs, hist, dim, lead), "lfi_stream_chunk_in", "null pointer (source 1)", "null source 1");
  expect(IN_ROWS(B, n, start, k, wins, no_second, seqs, hist, dim, lead), "lfi_stream_chunk_in_rows", "null pointer (source 1)",
         "null source 1");
  expect(ROLES_IN(B, n, start, k, wins, no_second, seqs, hist, dim, lead), "lfi_stream_chunk_roles_in", "null pointer (source 1)",
         "null generated source");
  // (gen_in takes a null source for it: with a device, tests/test_gpu_stream_windows.py)

  // lengths, roles, noise, out
  expect(lfi_stream_chunk_in_rows(B, n, start, k, wins, srcs, seqs, hist, dim, lead, guard, nullptr, nullptr), "lfi_stream_chunk_in_rows",
         "null pointer (lengths)", "null lengths");
  expect(lfi_stream_chunk_out_rows(B, n, start, k, wins, seqs, hist, dim, lead, nullptr, nullptr, nullptr), "lfi_stream_chunk_out_rows",
         "null pointer (lengths)", "null lengths");
  expect(lfi_stream_chunk_gen_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, gen, nullptr, C, guard, nullptr),
         "lfi_stream_chunk_gen_in", "null pointer (source table / noise)", "null noise");
  expect(lfi_stream_chunk_roles_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, gen, nullptr, C, roles, guard, nullptr),
         "lfi_stream_chunk_roles_in", "null pointer (source table / noise)", "null noise");
  expect(lfi_stream_chunk_roles_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, gen, dev, C, nullptr, guard, nullptr),
         "lfi_stream_chunk_roles_in", "null pointer (roles)", "null roles");
  expect(lfi_stream_chunk_gen_out(B, n, start, k, wins, seqs, hist, dim, lead, gen, nullptr, ld, nullptr, guard, nullptr),
         "lfi_stream_chunk_gen_out", "null pointer (out)", "null out");

  // gen_win out of range, the noise width, the out pitch
  for (int bad : {-1, 2}) {
    expect(lfi_stream_chunk_gen_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, bad, dev, C, guard, nullptr),
           "lfi_stream_chunk_gen_in", "generated window", "gen_win out of range");
    expect(lfi_stream_chunk_roles_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, bad, dev, C, roles, guard, nullptr),
           "lfi_stream_chunk_roles_in", "generated window", "gen_win out of range");
    expect(lfi_stream_chunk_gen_out(B, n, start, k, wins, seqs, hist, dim, lead, bad, dev, ld, nullptr, guard, nullptr),
           "lfi_stream_chunk_gen_out", "generated window", "gen_win out of range");
  }
  expect(lfi_stream_chunk_gen_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, 0, dev, C, guard, nullptr), "lfi_stream_chunk_gen_in",
         "generated window 0 has dim 5, the noise C = 6", "noise width");
  expect(lfi_stream_chunk_roles_in(B, n, start, k, wins, srcs, seqs, hist, dim, lead, 0, dev, C, roles, guard, nullptr),
         "lfi_stream_chunk_roles_in", "generated window 0 has dim 5, the noise C = 6", "noise width");
  expect(lfi_stream_chunk_gen_out(B, n, start, k, wins, seqs, hist, dim, lead, gen, dev, ld - 1, nullptr, guard, nullptr),
         "lfi_stream_chunk_gen_out", "out row pitch 17 below the 3 frames' 18 floats", "ld_out too small");

  std::printf("%d cases, %d missed\n", g_cases, g_missed);
  return g_missed ? 1 : 0;
}
