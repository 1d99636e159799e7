// Stand-alone driver of the host C ABI (common.cpp, sampler.cpp, loader.cpp), linked with their objects and compiled with
// them under -fsanitize (make -C selfrec_amd/csrc host_san).  No shared library, no dlopen, no python, no device work.
//
//   host_driver --about                       which sanitizers this binary was compiled with
//   host_driver run OUT_DIR SCRIPT [SCRIPT..] one script: run it, write OUT_DIR/index.txt and OUT_DIR/<buffer>.bin
//                                             several: one thread per script, all released together; script k writes OUT_DIR/t<k>/
//
// A script is a text file, one command per line, tokens separated by blanks (tests/test_host_sanitized_cpu.py writes them and
// runs the same lines against the production library through ctypes):
//   setenv NAME VALUE                 (single-script runs only: the library reads its thread counts with getenv)
//   buf NAME DTYPE COUNT              zeroed array of exactly COUNT elements (a heap block of its own: ASan sees its ends)
//   load NAME DTYPE PATH              private copy of a raw little-endian file
//   share NAME DTYPE PATH             the file's bytes, read once before any thread starts and shared by every script
//   call LABEL FUNCTION ARG..         one C ABI call; its status and, when it is not 0, srh_last_error_string() are recorded
// DTYPE: i32 u32 i64 f32 f64 u8.  COUNT: terms joined by '+': an integer, NAME[k] (element k of an integer array) or $LABEL
// (the value an earlier call returned).  ARG: i:<integer>  fb:<float32 bit pattern>  s:<string>  @NAME (the array's address)
// h:NAME (a handle)  &h:NAME (where a create call stores it)  null.
// index.txt: "A name dtype count" per array (every array the script owns is written out), "S label status message" per call.
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "selfrec_hip.h"

#ifndef __has_feature
#define __has_feature(x) 0
#endif
#if __has_feature(address_sanitizer) || defined(__SANITIZE_ADDRESS__)
#define DRIVER_ASAN 1
#else
#define DRIVER_ASAN 0
#endif
#if __has_feature(thread_sanitizer) || defined(__SANITIZE_THREAD__)
#define DRIVER_TSAN 1
#else
#define DRIVER_TSAN 0
#endif
#if __has_feature(undefined_behavior_sanitizer)
#define DRIVER_UBSAN 1
#else
#define DRIVER_UBSAN 0
#endif

namespace {

[[noreturn]] void die(const std::string& why) {
  fprintf(stderr, "host_driver: %s\n", why.c_str());
  exit(2);
}

size_t elem_size(const std::string& dtype) {
  if (dtype == "i32" || dtype == "u32" || dtype == "f32") return 4;
  if (dtype == "i64" || dtype == "f64") return 8;
  if (dtype == "u8") return 1;
  die("unknown dtype " + dtype);
}

bool read_bytes(const std::string& path, std::vector<char>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) out.insert(out.end(), chunk, chunk + got);
  fclose(f);
  return true;
}

char* exact_block(size_t bytes) {          // one heap block of exactly `bytes` (never null: an empty array is not "no array")
  char* p = (char*)malloc(bytes);
  if (!p && bytes == 0) p = (char*)malloc(1);
  if (!p) die("out of memory");
  return p;
}

struct Buf {
  std::string dtype;
  size_t count = 0;
  char* p = nullptr;
  bool owned = true;
};

struct SharedFile { char* p; size_t bytes; };
std::map<std::string, SharedFile> g_shared;          // filled by main before any script runs, read-only afterwards

struct Ctx {
  std::vector<std::vector<std::string>> lines;
  std::map<std::string, Buf> bufs;
  std::vector<std::string> order;
  std::map<std::string, void*> handles;
  std::map<std::string, long long> returned;
  std::string index, out_dir;
  bool may_setenv = true;

  Buf& buf(const std::string& name) {
    auto it = bufs.find(name);
    if (it == bufs.end()) die("no array " + name);
    return it->second;
  }
  void add(const std::string& name, Buf b) {
    if (bufs.count(name)) die("array " + name + " defined twice");
    bufs[name] = b;
    order.push_back(name);
  }
  long long count_of(const std::string& expr) {
    long long total = 0;
    size_t at = 0;
    while (at <= expr.size()) {
      size_t plus = expr.find('+', at);
      if (plus == std::string::npos) plus = expr.size();
      const std::string term = expr.substr(at, plus - at);
      if (term.empty()) die("bad count " + expr);
      if (term[0] == '$') {
        auto it = returned.find(term.substr(1));
        if (it == returned.end()) die("no call " + term);
        total += it->second;
      } else if (term.find('[') != std::string::npos) {
        const size_t lb = term.find('[');
        Buf& b = buf(term.substr(0, lb));
        const size_t k = (size_t)strtoull(term.c_str() + lb + 1, nullptr, 10);
        if (k >= b.count) die("count index out of range in " + expr);
        if (b.dtype == "i64") total += ((const int64_t*)b.p)[k];
        else if (b.dtype == "i32") total += ((const int32_t*)b.p)[k];
        else die("count from a non-integer array in " + expr);
      } else {
        total += strtoll(term.c_str(), nullptr, 10);
      }
      at = plus + 1;
    }
    if (total < 0) die("negative count " + expr);
    return total;
  }

  // ---- arguments
  static const std::string& need(const std::vector<std::string>& a, size_t k) {
    if (k >= a.size()) die("too few arguments");
    return a[k];
  }
  int64_t I(const std::vector<std::string>& a, size_t k) {
    const std::string& t = need(a, k);
    if (t.compare(0, 2, "i:") != 0) die("expected i:<integer>, got " + t);
    return t[2] == '-' ? (int64_t)strtoll(t.c_str() + 2, nullptr, 10) : (int64_t)strtoull(t.c_str() + 2, nullptr, 10);
  }
  float F(const std::vector<std::string>& a, size_t k) {
    const std::string& t = need(a, k);
    if (t.compare(0, 3, "fb:") != 0) die("expected fb:<bits>, got " + t);
    const uint32_t bits = (uint32_t)strtoul(t.c_str() + 3, nullptr, 10);
    float f;
    memcpy(&f, &bits, 4);
    return f;
  }
  void* P(const std::vector<std::string>& a, size_t k) {
    const std::string& t = need(a, k);
    if (t == "null") return nullptr;
    if (t[0] != '@') die("expected @array or null, got " + t);
    return buf(t.substr(1)).p;
  }
  void* H(const std::vector<std::string>& a, size_t k) {
    const std::string& t = need(a, k);
    if (t == "null") return nullptr;
    if (t.compare(0, 2, "h:") != 0) die("expected h:<handle> or null, got " + t);
    return handles[t.substr(2)];
  }
  void** HP(const std::vector<std::string>& a, size_t k) {
    const std::string& t = need(a, k);
    if (t == "null") return nullptr;
    if (t.compare(0, 3, "&h:") != 0) die("expected &h:<handle> or null, got " + t);
    return &handles[t.substr(3)];
  }
  const char* S(const std::vector<std::string>& a, size_t k) {
    const std::string& t = need(a, k);
    if (t == "null") return nullptr;
    if (t.compare(0, 2, "s:") != 0) die("expected s:<string> or null, got " + t);
    return t.c_str() + 2;
  }

  long long call(const std::string& fn, const std::vector<std::string>& a) {
    typedef int32_t* pi32;
    typedef int64_t* pi64;
    if (fn == "srh_sampler_create")
      return srh_sampler_create((srh_sampler_t**)HP(a, 0), I(a, 1), I(a, 2), I(a, 3), (pi32)P(a, 4), (pi32)P(a, 5));
    if (fn == "srh_sampler_destroy") {
      srh_sampler_destroy((srh_sampler_t*)H(a, 0));
      if (need(a, 0) != "null") handles[a[0].substr(2)] = nullptr;
      return 0;
    }
    if (fn == "srh_sampler_set_state")
      return srh_sampler_set_state((srh_sampler_t*)H(a, 0), (const uint32_t*)P(a, 1), (int32_t)I(a, 2));
    if (fn == "srh_sampler_get_state") return srh_sampler_get_state((srh_sampler_t*)H(a, 0), (uint32_t*)P(a, 1), (pi32)P(a, 2));
    if (fn == "srh_sampler_seed") return srh_sampler_seed((srh_sampler_t*)H(a, 0), (uint64_t)I(a, 1));
    if (fn == "srh_sampler_shuffle") return srh_sampler_shuffle((srh_sampler_t*)H(a, 0));
    if (fn == "srh_sampler_get_order") return srh_sampler_get_order((srh_sampler_t*)H(a, 0), (pi64)P(a, 1));
    if (fn == "srh_sampler_next_batch")
      return srh_sampler_next_batch((srh_sampler_t*)H(a, 0), I(a, 1), I(a, 2), (int32_t)I(a, 3), (pi32)P(a, 4), (pi32)P(a, 5),
                                    (pi32)P(a, 6), (pi64)P(a, 7));
    if (fn == "srh_sampler_epoch")
      return srh_sampler_epoch((srh_sampler_t*)H(a, 0), I(a, 1), (int32_t)I(a, 2), (pi32)P(a, 3), (pi32)P(a, 4), (pi32)P(a, 5),
                               (pi32)P(a, 6), (pi32)P(a, 7), (pi32)P(a, 8), (pi32)P(a, 9));
    if (fn == "srh_sampler_epoch_segments")
      return srh_sampler_epoch_segments((srh_sampler_t*)H(a, 0), I(a, 1), (pi32)P(a, 2), (pi32)P(a, 3), (pi32)P(a, 4),
                                        (pi32)P(a, 5), (pi32)P(a, 6), (pi32)P(a, 7), (pi32)P(a, 8), (int32_t)I(a, 9),
                                        (int32_t)I(a, 10), (pi32)P(a, 11), (pi32)P(a, 12), (pi32)P(a, 13), (pi32)P(a, 14),
                                        (pi32)P(a, 15), (pi32)P(a, 16));
    if (fn == "srh_sampler_sample_range") return srh_sampler_sample_range((srh_sampler_t*)H(a, 0), I(a, 1), I(a, 2), (pi64)P(a, 3));
    if (fn == "srh_sampler_next_u32") return srh_sampler_next_u32((srh_sampler_t*)H(a, 0), (uint32_t*)P(a, 1));
    if (fn == "srh_find_k_largest_host")
      return srh_find_k_largest_host(I(a, 0), (const float*)P(a, 1), I(a, 2), (pi64)P(a, 3), (float*)P(a, 4), (pi64)P(a, 5));
    if (fn == "srh_find_k_largest_host_f64")
      return srh_find_k_largest_host_f64(I(a, 0), (const double*)P(a, 1), I(a, 2), (pi64)P(a, 3), (double*)P(a, 4), (pi64)P(a, 5));
    if (fn == "srh_mt19937_uniform_f32")
      return srh_mt19937_uniform_f32((uint32_t*)P(a, 0), (pi32)P(a, 1), I(a, 2), (float*)P(a, 3), F(a, 4), (uint8_t*)P(a, 5));
    if (fn == "srh_dataset_load") return srh_dataset_load((srh_dataset_t**)HP(a, 0), S(a, 1), S(a, 2));
    if (fn == "srh_dataset_destroy") {
      srh_dataset_destroy((srh_dataset_t*)H(a, 0));
      if (need(a, 0) != "null") handles[a[0].substr(2)] = nullptr;
      return 0;
    }
    if (fn == "srh_dataset_sizes") return srh_dataset_sizes((srh_dataset_t*)H(a, 0), (pi64)P(a, 1));
    if (fn == "srh_dataset_copy_ids")
      return srh_dataset_copy_ids((srh_dataset_t*)H(a, 0), (pi32)P(a, 1), (pi32)P(a, 2), (float*)P(a, 3), (pi32)P(a, 4), (pi32)P(a, 5));
    if (fn == "srh_dataset_names_bytes") return srh_dataset_names_bytes((srh_dataset_t*)H(a, 0), (int32_t)I(a, 1));
    if (fn == "srh_dataset_copy_names") return srh_dataset_copy_names((srh_dataset_t*)H(a, 0), (int32_t)I(a, 1), (char*)P(a, 2), (pi64)P(a, 3));
    die("unknown function " + fn);
  }

  void run() {
    for (const auto& t : lines) {
      const std::string& cmd = t[0];
      if (cmd == "setenv") {
        if (!may_setenv) die("setenv beside other threads");
        setenv(need(t, 1).c_str(), need(t, 2).c_str(), 1);
      } else if (cmd == "buf") {
        Buf b;
        b.dtype = need(t, 2);
        b.count = (size_t)count_of(need(t, 3));
        const size_t bytes = b.count * elem_size(b.dtype);
        b.p = exact_block(bytes);
        if (bytes) memset(b.p, 0, bytes);
        add(need(t, 1), b);
      } else if (cmd == "load" || cmd == "share") {
        auto it = g_shared.find(need(t, 3));
        if (it == g_shared.end()) die("file was not read: " + t[3]);
        Buf b;
        b.dtype = need(t, 2);
        if (it->second.bytes % elem_size(b.dtype)) die("file size is no multiple of the element size: " + t[3]);
        b.count = it->second.bytes / elem_size(b.dtype);
        if (cmd == "share") {
          b.p = it->second.p;
          b.owned = false;
        } else {
          b.p = exact_block(it->second.bytes);
          if (it->second.bytes) memcpy(b.p, it->second.p, it->second.bytes);
        }
        add(need(t, 1), b);
      } else if (cmd == "call") {
        const std::string& label = need(t, 1);
        const std::vector<std::string> args(t.begin() + std::min<size_t>(3, t.size()), t.end());
        const long long rc = call(need(t, 2), args);
        returned[label] = rc;
        index += "S " + label + " " + std::to_string(rc);
        if (rc < 0) index += std::string(" ") + srh_last_error_string();
        index += "\n";
      } else {
        die("unknown command " + cmd);
      }
    }
  }

  void write_out() {
    for (const auto& h : handles)
      if (h.second) die("handle " + h.first + " was not destroyed");
    std::string head;
    for (const std::string& name : order) {
      Buf& b = bufs[name];
      if (!b.owned) continue;
      head += "A " + name + " " + b.dtype + " " + std::to_string(b.count) + "\n";
      FILE* f = fopen((out_dir + "/" + name + ".bin").c_str(), "wb");
      if (!f) die("cannot write into " + out_dir);
      const size_t bytes = b.count * elem_size(b.dtype);
      if (bytes && fwrite(b.p, 1, bytes, f) != bytes) die("short write");
      fclose(f);
    }
    FILE* f = fopen((out_dir + "/index.txt").c_str(), "wb");
    if (!f) die("cannot write into " + out_dir);
    fputs((head + index).c_str(), f);
    fclose(f);
    for (auto& kv : bufs)
      if (kv.second.owned) free(kv.second.p);
  }
};

void parse(const std::string& path, Ctx& c) {
  std::vector<char> text;
  if (!read_bytes(path, text)) die("cannot read " + path);
  std::vector<std::string> tokens;
  std::string cur;
  auto end_token = [&] { if (!cur.empty()) { tokens.push_back(cur); cur.clear(); } };
  auto end_line = [&] {
    end_token();
    if (!tokens.empty()) c.lines.push_back(tokens);
    tokens.clear();
  };
  for (char ch : text) {
    if (ch == '\n') end_line();
    else if (ch == ' ' || ch == '\t' || ch == '\r') end_token();
    else cur.push_back(ch);
  }
  end_line();
  for (const auto& t : c.lines)
    if ((t[0] == "load" || t[0] == "share") && t.size() >= 4 && !g_shared.count(t[3])) {
      std::vector<char> bytes;
      if (!read_bytes(t[3], bytes)) die("cannot read " + t[3]);
      SharedFile sf{exact_block(bytes.size()), bytes.size()};
      if (!bytes.empty()) memcpy(sf.p, bytes.data(), bytes.size());
      g_shared[t[3]] = sf;
    }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--about") {
    std::string s = "sanitizers:";
    if (DRIVER_ASAN) s += " address";
    if (DRIVER_UBSAN) s += " undefined";
    if (DRIVER_TSAN) s += " thread";
    if (!DRIVER_ASAN && !DRIVER_UBSAN && !DRIVER_TSAN) s += " none";
    puts(s.c_str());
    return 0;
  }
  if (argc < 4 || std::string(argv[1]) != "run") die("usage: host_driver --about | host_driver run OUT_DIR SCRIPT [SCRIPT..]");
  const int n = argc - 3;
  std::vector<Ctx> ctx((size_t)n);
  for (int k = 0; k < n; ++k) {
    parse(argv[3 + k], ctx[(size_t)k]);
    ctx[(size_t)k].out_dir = n == 1 ? std::string(argv[2]) : std::string(argv[2]) + "/t" + std::to_string(k);
    ctx[(size_t)k].may_setenv = n == 1;
  }
  if (n == 1) {
    ctx[0].run();
  } else {
    std::mutex mu;
    std::condition_variable cv;
    int ready = 0;
    std::vector<std::thread> pool;
    for (int k = 0; k < n; ++k)
      pool.emplace_back([&, k] {
        {
          std::unique_lock<std::mutex> lock(mu);          // every script starts at the same moment
          if (++ready == n) cv.notify_all();
          else cv.wait(lock, [&] { return ready == n; });
        }
        ctx[(size_t)k].run();
      });
    for (auto& th : pool) th.join();
  }
  for (auto& c : ctx) c.write_out();
  for (auto& kv : g_shared) free(kv.second.p);
  return 0;
}
