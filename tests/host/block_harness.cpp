// block_harness.cpp -- the owner of csrc/mrs_tg_block.hpp (every device block a plan, a context or a scope keeps) compiled with
// plain g++ over a counting allocator that can be told to fail: the states behind a failed allocation, a failed fill and a
// failed idle step, which no GPU test may provoke.  tests/test_block_host.py builds and runs it, plain and under sanitizers.
//
//   g++ -std=c++17 -O2 tests/host/block_harness.cpp -o block_harness && ./block_harness
//
// No input.  One output line per check, "ok <name>", and exit code 0; the first failed check prints "FAIL <name>: <what>" and
// exits with 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_block.hpp"

namespace {

enum Err { kOk = 0, kNoMemory = 2, kStreamFaulted = 7, kFillFailed = 9 };

struct Fake {
  using Error = Err;
  static constexpr Err ok = kOk;
  static int live;                      // blocks handed out and not yet given back
  static int allocs;                    // calls of alloc so far
  static int fail_at;                   // the allocs-th call (1-based) fails; 0: none
  static Err idle_says;                 // what the default idle step returns
  static std::vector<std::string> log;  // "idle", "free", "alloc <bytes>" in the order they happened
  static Err alloc(void** p, size_t bytes) {
    if (++allocs == fail_at) {
      log.push_back("alloc-failed");
      return kNoMemory;  // (*p is left alone: the owner must not read it)
    }
    *p = std::malloc(bytes);
    ++live;
    log.push_back("alloc " + std::to_string(bytes));
    return kOk;
  }
  static void free(void* p) {
    std::free(p);
    --live;
    log.push_back("free");
  }
  static Err idle() {
    log.push_back("idle");
    return idle_says;
  }
  static void reset() {
    live = allocs = fail_at = 0;
    idle_says = kOk;
    log.clear();
  }
};
int Fake::live, Fake::allocs, Fake::fail_at;
Err Fake::idle_says;
std::vector<std::string> Fake::log;

template <class T>
using Blk = mrs_tg::Block<T, Fake>;

static_assert(!std::is_copy_constructible<Blk<int>>::value && !std::is_copy_assignable<Blk<int>>::value &&
                  !std::is_move_constructible<Blk<int>>::value,
              "one owner per block");

const char* g_name = "";
void begin(const char* name) {
  g_name = name;
  Fake::reset();
}
void end() {
  if (Fake::live != 0) {
    std::printf("FAIL %s: %d blocks live after every owner left its scope\n", g_name, Fake::live);
    std::exit(1);
  }
  std::printf("ok %s\n", g_name);
}
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s: %s (line %d)\n", g_name, #cond, __LINE__); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

bool log_is(std::vector<std::string> want) { return Fake::log == want; }
template <class T>
bool empty(const Blk<T>& b) {
  return b.get() == nullptr && b.count() == 0;
}

}  // namespace

int main() {
  begin("ensure_allocates_once_and_grows_behind_idle");
  {
    Blk<double> b;
    CHECK(empty(b));
    CHECK(b.ensure(10) == kOk && b.get() && b.count() == 10);
    b.get()[9] = 1.0;  // (the sanitizers check the size)
    CHECK(log_is({"alloc 80"}));
    double* const first = b.get();
    CHECK(b.ensure(10) == kOk && b.ensure(3) == kOk && b.ensure(0) == kOk);
    CHECK(b.get() == first && b.count() == 10 && log_is({"alloc 80"}));
    CHECK(b.ensure(11) == kOk && b.count() == 11);
    b.get()[10] = 1.0;
    CHECK(log_is({"alloc 80", "idle", "free", "alloc 88"}));
    CHECK(Fake::live == 1);
  }
  CHECK(Fake::log.back() == "free");
  end();

  begin("caller_idle_step_and_headroom");
  {
    Blk<char> b;
    int waited = 0;
    auto idle = [&] {
      ++waited;
      Fake::log.push_back("caller-idle");
      return kOk;
    };
    CHECK(b.ensure(100, idle, 100 / 4) == kOk && b.count() == 125 && waited == 0);  // an empty block waits for nothing
    CHECK(b.ensure(125, idle, 125 / 4) == kOk && waited == 0 && Fake::allocs == 1);  // within the headroom
    CHECK(b.ensure(126, idle, 126 / 2) == kOk && b.count() == 189 && waited == 1);
    CHECK(log_is({"alloc 125", "caller-idle", "free", "alloc 189"}));
  }
  end();

  begin("failed_allocation_leaves_the_block_empty");
  {
    Blk<int> b;
    Fake::fail_at = 1;
    CHECK(b.ensure(5) == kNoMemory && empty(b) && Fake::live == 0);
    CHECK(b.ensure(5) == kOk && b.count() == 5 && Fake::live == 1);
    // growing: the old block is gone, the new one did not come, the block is empty and says so
    Fake::fail_at = Fake::allocs + 1;
    CHECK(b.ensure(6) == kNoMemory && empty(b) && Fake::live == 0);
    CHECK(b.ensure(6) == kOk && b.count() == 6);
  }
  end();

  begin("pair_both_held_or_both_empty");  // d_H / d_Ainv: the second allocation fails
  {
    Blk<double> h, ainv;
    Fake::fail_at = 2;
    CHECK(mrs_tg::ensure_both(h, 100, ainv, 100) == kNoMemory);
    CHECK(empty(h) && empty(ainv) && Fake::live == 0);
    CHECK(log_is({"alloc 800", "alloc-failed", "free"}));
    CHECK(mrs_tg::ensure_both(h, 100, ainv, 100) == kOk && h.holds(100) && ainv.holds(100) && Fake::live == 2);
    const int allocs = Fake::allocs;
    CHECK(mrs_tg::ensure_both(h, 100, ainv, 100) == kOk && Fake::allocs == allocs);  // both held: nothing happens
    Fake::fail_at = Fake::allocs + 1;  // the first fails
    Blk<double> c, d;
    CHECK(mrs_tg::ensure_both(c, 1, d, 1) == kNoMemory && empty(c) && empty(d) && Fake::live == 2);
  }
  end();

  begin("filled_once_fill_failure_empties_the_block");  // d_careful, d_dfo_seg_path
  {
    Blk<int> b;
    int fills = 0;
    Err fill_says = kFillFailed;
    auto fill = [&](int* p) {
      ++fills;
      p[3] = 0;
      return fill_says;
    };
    CHECK(b.ensure_filled(4, fill) == kFillFailed && fills == 1 && empty(b) && Fake::live == 0);
    fill_says = kOk;
    CHECK(b.ensure_filled(4, fill) == kOk && fills == 2 && b.holds(4) && Fake::live == 1);  // allocated and filled again
    CHECK(b.ensure_filled(4, fill) == kOk && fills == 2 && Fake::allocs == 2);              // held: no fill, no allocation
    Fake::fail_at = Fake::allocs + 1;
    Blk<int> c;
    CHECK(c.ensure_filled(4, fill) == kNoMemory && fills == 2 && empty(c));  // nothing to fill
  }
  end();

  begin("failing_idle_is_returned_old_block_freed_nothing_allocated");  // the workspace of a plan whose stream has faulted
  {
    Blk<double> b;
    CHECK(b.ensure(4) == kOk);
    CHECK(b.ensure(8, [] {
      Fake::log.push_back("caller-idle");
      return kStreamFaulted;
    }) == kStreamFaulted);
    CHECK(empty(b) && Fake::live == 0 && Fake::allocs == 1);
    CHECK(log_is({"alloc 32", "caller-idle", "free"}));
    CHECK(b.ensure(4) == kOk);
    Fake::idle_says = kStreamFaulted;  // the allocator's own idle step, the default
    CHECK(b.ensure(8) == kStreamFaulted && empty(b) && Fake::live == 0 && Fake::allocs == 2);
    Fake::idle_says = kOk;
    CHECK(b.ensure(8) == kOk && b.holds(8));
  }
  end();

  begin("request_of_zero_is_a_request_of_one");
  {
    Blk<double> b;
    CHECK(!b.holds(0));
    CHECK(b.ensure(0) == kOk && b.get() && b.count() == 1 && log_is({"alloc 8"}));
    b.get()[0] = 1.0;
    CHECK(b.ensure(0) == kOk && b.ensure(1) == kOk && Fake::allocs == 1);
    Blk<char> c;
    CHECK(c.ensure_filled(0, [](char* p) { return *p = 0, kOk; }) == kOk && c.count() == 1);
    Blk<int> d, e;
    CHECK(mrs_tg::ensure_both(d, 0, e, 0) == kOk && d.count() == 1 && e.count() == 1 && Fake::live == 4);
  }
  end();

  begin("reset_gives_back_once");
  {
    Blk<int> b;
    b.reset();
    CHECK(Fake::log.empty());
    CHECK(b.ensure(2) == kOk);
    b.reset();
    b.reset();
    CHECK(empty(b) && log_is({"alloc 8", "free"}));
  }
  end();
  return 0;
}
