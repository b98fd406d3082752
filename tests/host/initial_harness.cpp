// initial_harness.cpp -- csrc/mrs_tg_initial.hpp (the bins, the decision table and the splice's plan and chunk walk that
// mrs_tg_initial.hip runs) compiled with plain g++ next to the public host header include/mrs_tg_initial_condition.hpp, and both
// asked the same questions.  tests/test_initial_host.py compares the answers; tests/test_gpu_initial.py holds the kernels to the
// public functions.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/initial_harness.cpp -o initial_harness && ./initial_harness < in
//
// Input, one problem per line, any number until end of input:
//   O x                                          -> sample_offset(x) of the new header, of the public one, splice_offset(x) of both
//   D tracker age uav dont offset n_wp n_pred    -> word k | has_initial_condition from_future drop_first k source rc
//        tracker: 1 a tracker command is present; uav: 1 a UAV state is present; dont: dont_prepend.  The public function runs on
//        a tracker command whose x is 1, a UAV state whose x is 2 and a prediction whose row i has x = 100 + i; source says which
//        of them its waypoint is (8 tracker, 16 UAV, 32 prediction row k, 0 none -- the values of MRS_TG_IC_FROM_*); rc its
//        return code.  The new decide() runs with pred_capacity = 64.
//   S n k capacity                               -> count_public count_walk same_bytes
//        n sample rows, k prediction rows in front (age 0: the prediction's current index is 0), in a buffer of `capacity` rows
//        with 3 guard rows behind it: the public splice (memmove + memcpy) against a serial restatement of the kernel's in-place
//        walk -- chunks of 64 from the last to the first, a chunk's rows all loaded before one is stored, the prefix last.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mrs_tg_initial_condition.hpp"
#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_initial.hpp"

namespace pub = mrs_tg::initial_condition;
namespace iq = mrs_tg::initq;

static int offsets() {
  double x = 0.0;
  if (std::scanf("%lf", &x) != 1) return 2;
  std::printf("%d %d %d %d\n", iq::sample_offset(x), pub::sample_offset(x), iq::splice_offset(x), pub::splice_offset(x));
  return 0;
}

static int decision() {
  int tracker = 0, uav = 0, dont = 0, n_wp = 0, n_pred = 0;
  double age = 0.0, offset = 0.0;
  if (std::scanf("%d %lf %d %d %lf %d %d", &tracker, &age, &uav, &dont, &offset, &n_wp, &n_pred) != 7) return 2;
  const iq::Decision d = iq::decide(tracker != 0, age, uav != 0, dont != 0, offset, n_wp, n_pred, 64);
  mrs_tg_waypoint pose{};
  mrs_tg_initial_state state{};
  pose.coords[0] = 1.0, pose.coords[3] = 0.5, state.heading = 0.5, state.velocity[0] = 0.25;
  const double uav_pose[4] = {2.0, 0.0, 1.0, -0.5};
  const int rows = n_pred > 0 ? n_pred : 0;
  std::vector<double> pos((size_t)rows * 4 + 4, 0.0), zero((size_t)rows * 4 + 4, 0.0);
  for (int i = 0; i < rows; ++i) pos[(size_t)i * 4] = 100.0 + i;
  mrs_tg_prediction pred{n_pred, pos.data(), zero.data(), zero.data(), zero.data()};
  pub::Decision o;
  const char* why = "";
  const int rc = pub::prepare(tracker ? &pose : nullptr, tracker ? &state : nullptr, age, &pred, uav ? uav_pose : nullptr, 1.5, offset,
                              n_wp, dont != 0, &o, &why);
  int source = 0;
  if (rc == MRS_TG_OK && o.has_initial_condition) {
    const double x = o.waypoint.coords[0];
    source = x == 1.0 ? 8 : (x == 2.0 ? 16 : (x == 100.0 + o.sample_offset ? 32 : -1));
    if (source == 16 && o.waypoint.coords[2] != 2.5) source = -1;  // z + takeoff_height
  }
  std::printf("%d %d | %d %d %d %d %d %d\n", d.word, d.k, (int)o.has_initial_condition, (int)o.from_future,
              (int)o.drop_first_waypoint, o.sample_offset, source, rc);
  return 0;
}

static int splice() {
  int n = 0, k = 0, cap = 0;
  if (std::scanf("%d %d %d", &n, &k, &cap) != 3 || n < 0 || k < 0 || cap < 0) return 2;
  const int guard = 3;
  const size_t total = ((size_t)(cap > n ? cap : n) + guard) * 4;
  std::vector<double> a(total), pos((size_t)k * 4 + 4);
  for (size_t e = 0; e < total; ++e) a[e] = e < (size_t)n * 4 ? 0.25 + (double)e : -7.0 - (double)e;
  for (size_t e = 0; e < pos.size(); ++e) pos[e] = 1000.5 + (double)e;
  std::vector<double> b = a;
  std::vector<double> zero(pos.size(), 0.0);
  mrs_tg_prediction pred{k + 1, pos.data(), zero.data(), zero.data(), zero.data()};
  const char* why = "";
  const int count_public = pub::splice(&pred, k, 0.0, a.data(), n, cap, &why);
  // the kernel's walk, one "lane" after the other
  const iq::SplicePlan s = iq::splice_plan(true, n, cap, iq::kPrepend | iq::kFromFuture | iq::kFromPrediction, k, 0.0, k + 1);
  int count_walk = n;
  if (s.action == iq::kTooLong) count_walk = s.count;
  if (s.action == iq::kInsert) {
    count_walk = s.count;
    double held[iq::kSpliceChunk][4];
    for (int c = iq::splice_chunks(s.n) - 1; c >= 0; --c) {
      for (int lane = 0; lane < iq::kSpliceChunk; ++lane) {
        const int i = c * iq::kSpliceChunk + lane;
        if (i < s.n) std::memcpy(held[lane], &b[(size_t)i * 4], sizeof held[lane]);
      }
      for (int lane = 0; lane < iq::kSpliceChunk; ++lane) {
        const int i = c * iq::kSpliceChunk + lane;
        if (i < s.n) std::memcpy(&b[(size_t)(i + s.k) * 4], held[lane], sizeof held[lane]);
      }
    }
    for (int i = 0; i < s.k; ++i) std::memcpy(&b[(size_t)i * 4], &pos[(size_t)i * 4], 4 * sizeof(double));
  }
  std::printf("%d %d %d\n", count_public, count_walk, (int)(std::memcmp(a.data(), b.data(), total * sizeof(double)) == 0));
  return 0;
}

int main() {
  for (;;) {
    char what = 0;
    if (std::scanf(" %c", &what) != 1) return 0;
    int rc = 2;
    if (what == 'O') rc = offsets();
    if (what == 'D') rc = decision();
    if (what == 'S') rc = splice();
    if (rc != 0) return rc;
  }
}
