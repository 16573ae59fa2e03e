// tests/native/check_launch.hip -- what the update launchers would launch, recorded
// without a device (tests/test_launch_plan_cpu.py, tests/golden/launch_plan.txt).
//
// hipLaunchKernelGGL is redefined as a recorder before kernels.hip is included whole, so
// launch_update, launch_update_encode and launch_update_kardam run their own host code and
// every launch becomes one line: the kernel, the grid, the block and every argument.
// hipGetDevice / hipDeviceGetAttribute are redefined too: fake device i reports the i-th
// CU count of kCus (device_simds caches per device index), hipGetLastError reports success.
// Only names of kernels.h and of the kernels' argument structs are used, so the same file
// records any tree that keeps those launchers.
//
//   check_launch                 the fixture: one hash line per (spec, CUs, launcher)
//                                block, then the default spec's 256-CU lines with M = 64
//   check_launch --dump SPEC CUS every line of that spec's blocks (diff two trees with it)
//   check_launch --sizes         the sizes and specs covered
//
// Build: hipcc --offload-arch=gfx950 -O1 -std=c++17 -Ifleet_amd/csrc -Iinclude
//        tests/native/check_launch.hip [fleet_amd/csrc/launch_plan.cpp] -rdynamic -o check_launch
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

namespace rec {
constexpr int kCus[3] = {256, 304, 64};
int g_dev = 0;
std::string g_ctx, g_out;  // the current call's prefix; the current block's lines

hipError_t get_device(int* dev) {
  *dev = g_dev;
  return hipSuccess;
}
hipError_t get_attribute(int* v, hipDeviceAttribute_t, int dev) {
  *v = kCus[dev];
  return hipSuccess;
}
inline hipError_t last_error() { return hipSuccess; }

template <class... A>
void putf(const char* f, A... a) {
  char b[256];
  snprintf(b, sizeof b, f, a...);
  g_out += b;
}
// the kernel as the compiler resolved it (defaulted template arguments included), from the
// symbol of its host stub: "k_update_pipe<16, 1, 5, 0, false>" (link with -rdynamic)
template <class K>
std::string kernel(K* k) {
  Dl_info di;
  if (!dladdr(reinterpret_cast<void*>(k), &di) || !di.dli_sname) return "?";
  int st = 0;
  char* d = abi::__cxa_demangle(di.dli_sname, nullptr, nullptr, &st);
  std::string n = st == 0 && d ? d : di.dli_sname;
  free(d);
  for (const char* lead : {"fleet::", "__device_stub__"}) {  // drop "void fleet::"
    const size_t a = n.find(lead);
    if (a != std::string::npos) n = n.substr(a + strlen(lead));
  }
  int depth = 0;  // up to the parameter list
  for (size_t i = 0; i < n.size(); ++i) {
    if (n[i] == '<') ++depth;
    else if (n[i] == '>') --depth;
    else if (n[i] == '(' && depth == 0) return n.substr(0, i);
  }
  return n;
}
template <class T>
void arg(const T& v);
template <class... A>
void launch(const std::string& k, dim3 g, dim3 b, const A&... a) {
  g_out += g_ctx + " | " + k;
  putf(" grid=%u,%u block=%u args:", g.x, g.y, b.x);
  (arg(a), ...);
  g_out += "\n";
}
}  // namespace rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shmem, stream, ...) \
  rec::launch(rec::kernel(k), grid, block, __VA_ARGS__)
#define hipGetDevice rec::get_device
#define hipDeviceGetAttribute rec::get_attribute
#define hipGetLastError rec::last_error
#define FLEET_DEV_ALL_KERNELS 1
#include "kernels.hip"

namespace rec {
template <class T>
void arg(const T& v) {
  if constexpr (std::is_pointer<T>::value || std::is_null_pointer<T>::value) g_out += v ? " ptr" : " null";
  else if constexpr (std::is_integral<T>::value) putf(" %lld", (long long)v);
  else if constexpr (std::is_floating_point<T>::value) putf(" %a", (double)v);
  else if constexpr (std::is_same<T, fleet::EncodeJob>::value)
    putf(" EncodeJob{%s n=%lld vpitch=%zu %s pitch=%zu groups=%lld gx=%lld rows=%d rpb=%d prio=%d}",
         v.values ? "ptr" : "null", (long long)v.n, v.vpitch, v.out ? "ptr" : "null", v.pitch, (long long)v.groups,
         (long long)v.gx, v.rows, v.rpb, v.prio);
  else if constexpr (std::is_same<T, fleet::FlatGrid>::value)
    putf(" FlatGrid{nW=%d nU=%d w1=%d w2=%d}", v.nW, v.nU, v.w1, v.w2);
  else if constexpr (std::is_same<T, fleet::KardamReduceJob>::value)
    putf(" KardamReduceJob{%s %s epoch=%u wait_skew=%u}", v.norms ? "ptr" : "null", v.flags ? "ptr" : "null", v.epoch,
         v.wait_skew);
  else if constexpr (std::is_same<T, fleet::KardamOut>::value)
    putf(" KardamOut{lr=%a %s %s vpitch=%zu %s %s}", v.lr, v.prev ? "ptr" : "null", v.has_prev ? "ptr" : "null",
         v.vpitch, v.g_out ? "ptr" : "null", v.partials ? "ptr" : "null");
  else g_out += " <struct>";  // the launchers this program never calls
}

// GRID_SIZES of tests/test_capi_cpu.py, both sides of every boundary of its DEFAULT_PLAN,
// and of the CU-dependent rules for 304 and 64 CUs (three 64-group tiles per CU; the fused
// stream step's balanced split below 1024 groups per CU)
const long long kSizes[] = {
    1, 2, 16, 17, 83, 84, 85, 255, 256, 257, 1000, 6667, 7654, 12288, 12289, 14335, 14336, 16668, 24575, 24576, 32767,
    32768, 40959, 40960, 49152, 49153, 50001, 58368, 58369, 65535, 65536, 65537, 100001, 104623, 110413, 131071,
    131072, 174763, 262143, 262144, 311295, 311296, 349526, 1398102};
const int kRows[] = {1, 23, 24, 25, 64, 256};
// the specs of test_launch_grid_covers_every_group, then the encode side's
const char* const kSpecs[] = {"", "update=stream", "update=stream,grid=plain", "update=stream,grid=lanes",
                              "update=tiled", "update=tiled,tile=classic", "update=pipe", "update=tiled,tile=weave6",
                              "update=tiled,tile=weave8", "update=tiled,tile=flat", "update=tiled,tile=flat,flat_w2=16",
                              "update=tiled,tile=flat,flat_w2=64", "update=tiled,tile=flat,flat_w2=21", "fused=off",
                              "grid=balanced", "tile_enc_rows=7", "tile_enc_prio=2", "update=pipe,fused=off"};
const char* const kLaunchers[] = {"update", "update_encode", "update_kardam", "names"};

template <class T>
T* fake(int k) {  // a non-null pointer that is never followed
  return reinterpret_cast<T*>((uintptr_t)0x1000 * k);
}

void ctx(const char* what, long long groups, int M, long long g_begin) {
  char b[128];
  snprintf(b, sizeof b, "%s groups=%lld M=%d g_begin=%lld", what, groups, M, g_begin);
  g_ctx = b;
}

// one (spec, device, launcher) block into g_out; the overrides are set by the caller
void block(int launcher) {
  g_out.clear();
  for (long long groups : kSizes) {
    if (launcher == 3) {
      int kind = -1;
      int64_t blocks = -1, n_a = -1, n_w = -1, n_n = -1;
      fleet::update_plan_grid(groups, &kind, &blocks, &n_a, &n_w, &n_n);
      ctx("names", groups, 0, 0);
      g_out += g_ctx + " | update=" + fleet::update_kernel_name(groups) +
               " | update_encode=" + fleet::update_encode_kernel_name(groups);
      putf(" | kind=%d blocks=%lld n_a=%lld n_w=%lld n_n=%lld\n", kind, (long long)blocks, (long long)n_a,
           (long long)n_w, (long long)n_n);
      continue;
    }
    for (int M : kRows)
      for (long long g_begin : {0LL, 5LL}) {
        // a ragged last group; the window variant sits inside a longer upload
        const int64_t n_up = g_begin ? 3 * (groups + g_begin + 7) - 2 : 3 * groups - 1;
        const size_t pitch = (size_t)(16 * ((n_up + 2) / 3) + 16);
        const double inv = 1.0 / M;
        if (launcher == 0) {
          ctx("update", groups, M, g_begin);
          const hipError_t e = fleet::launch_update(fake<uint8_t>(1), pitch, M, fake<double>(2), inv, n_up, g_begin,
                                                    g_begin + groups, fake<int32_t>(3), fake<uint8_t>(4),
                                                    fake<float>(5), fake<int>(6), nullptr);
          g_out += g_ctx;
          putf(" | ret=%d\n", (int)e);
        } else if (launcher == 1) {
          if (g_begin) continue;  // it takes the whole upload
          ctx("update_encode", groups, M, 0);
          const hipError_t e = fleet::launch_update_encode(fake<uint8_t>(1), pitch, M, fake<double>(2), inv, n_up,
                                                           fake<int32_t>(3), fake<uint8_t>(4), fake<float>(5),
                                                           fake<int>(6), fake<float>(7), (size_t)n_up + 1,
                                                           fake<uint8_t>(8), nullptr);
          g_out += g_ctx;
          putf(" | ret=%d\n", (int)e);
        } else {
          const fleet::PlanOverrides o = fleet::plan_overrides();
          for (int sizing = 1; sizing >= 0; --sizing) {
            ctx(sizing ? "update_kardam(sizing)" : "update_kardam", groups, M, g_begin);
            const fleet::KardamOut kd{0.125, fake<float>(9), fake<uint8_t>(10), (size_t)n_up + 1, fake<float>(11),
                                      sizing ? nullptr : fake<double>(12)};
            int n_waves = -1, norm_parts = -1, flag_slots = -1;
            const hipError_t e = fleet::launch_update_kardam(
                fake<uint8_t>(1), pitch, M, fake<double>(2), inv, n_up, g_begin, g_begin + groups, fake<int32_t>(3),
                fake<uint8_t>(4), fake<float>(5), fake<int>(6), kd, &n_waves, sizing ? nullptr : fake<double>(13),
                &norm_parts, &flag_slots, sizing ? nullptr : fake<uint32_t>(14), 77u, o, nullptr, 0);
            g_out += g_ctx;
            putf(" | ret=%d n_waves=%d norm_parts=%d flag_slots=%d\n", (int)e, n_waves, norm_parts, flag_slots);
          }
        }
      }
  }
}

uint64_t fnv1a(const std::string& s) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char c : s) h = (h ^ c) * 0x100000001b3ull;
  return h;
}

size_t count_lines(const std::string& s) {
  size_t n = 0;
  for (char c : s) n += c == '\n';
  return n;
}

int set_spec(const char* spec) {
  std::string err;
  if (fleet::set_plan_overrides(spec, &err) != 0) {
    fprintf(stderr, "spec '%s' rejected: %s\n", spec, err.c_str());
    return -1;
  }
  return 0;
}
}  // namespace rec

int main(int argc, char** argv) {
  using namespace rec;
  if (argc == 2 && !strcmp(argv[1], "--sizes")) {
    printf("sizes");
    for (long long g : kSizes) printf(" %lld", g);
    printf("\nrows");
    for (int m : kRows) printf(" %d", m);
    printf("\ncus");
    for (int c : kCus) printf(" %d", c);
    printf("\n");
    for (const char* s : kSpecs) printf("spec %s\n", s);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "--dump")) {
    if (set_spec(argv[2]) != 0) return 2;
    for (g_dev = 0; g_dev < 3 && kCus[g_dev] != atoi(argv[3]); ++g_dev) {}
    if (g_dev == 3) return 2;
    for (int l = 0; l < 4; ++l) {
      block(l);
      fputs(g_out.c_str(), stdout);
    }
    return 0;
  }
  if (argc != 1) return 2;
  std::string full;
  for (const char* spec : kSpecs) {
    if (set_spec(spec) != 0) return 2;
    for (g_dev = 0; g_dev < 3; ++g_dev)
      for (int l = 0; l < 4; ++l) {
        block(l);
        printf("hash spec=%s cus=%d %s %016llx lines=%zu\n", *spec ? spec : "default", kCus[g_dev], kLaunchers[l],
               (unsigned long long)fnv1a(g_out), count_lines(g_out));
        if (*spec || g_dev != 0) continue;
        size_t p = 0;  // the default plan at 256 CUs: the lines of M = 64 (and the names) in full
        while (p < g_out.size()) {
          const size_t q = g_out.find('\n', p) + 1;
          const std::string ln = g_out.substr(p, q - p);
          if (l == 3 || ln.find(" M=64 ") != std::string::npos) full += ln;
          p = q;
        }
      }
  }
  fputs(full.c_str(), stdout);
  return 0;
}
