// emb_stat_rows, emb_mean_fill: the metrics of imag_loss (dreamerv3/agent.py:424-442)
// and the loss means of Agent.loss (dreamerv3/agent.py:239-240) with their
// backward, one launch per kStatMaxEntries entries (stat_rows.hip).  Its own
// translation unit, as optim_abi.cpp: kernels_abi.cpp is also linked into the
// host sanitizer soak, against stand-in launchers that know nothing of these
// kernels.
#include "abi_common.h"
#include "stat_rows.h"

using namespace emb_abi;

extern "C" {

int32_t emb_stat_rows(const emb_stat_entry_t* entries, int64_t count, void* out, void* total, void* stream) {
  return guarded([&] {
    const char* wrong = emb::stat_rows_error(entries, count, out, total);      // before any HIP call
    need(!wrong, wrong);
    float* row = static_cast<float*>(out);
    for (int64_t first = 0; first < count; first += emb::kStatMaxEntries) {
      const int n = static_cast<int>(std::min<int64_t>(count - first, emb::kStatMaxEntries));
      emb::StatTable table{};
      for (int k = 0; k < n; ++k) table.e[k] = emb::stat_entry_of(entries[first + k]);
      HIP_OK(emb::launch_stat_rows(table, n, row + first * emb::kStatValues, static_cast<float*>(total),
                                   static_cast<hipStream_t>(stream)));
    }
  });
}

int32_t emb_mean_fill(const emb_fill_entry_t* entries, int64_t count, const void* g, void* stream) {
  return guarded([&] {
    const char* wrong = emb::mean_fill_error(entries, count, g);               // before any HIP call
    need(!wrong, wrong);
    for (int64_t first = 0; first < count; first += emb::kStatMaxEntries) {
      const int n = static_cast<int>(std::min<int64_t>(count - first, emb::kStatMaxEntries));
      emb::FillTable table{};
      for (int k = 0; k < n; ++k) table.e[k] = entries[first + k];
      HIP_OK(emb::launch_mean_fill(table, n, static_cast<const float*>(g), static_cast<hipStream_t>(stream)));
    }
  });
}

int32_t emb_stat_rows_launches(int64_t* count) {
  return guarded([&] {
    need(count, "stat_rows_launches: count is null");
    *count = emb::stat_rows_launches();
  });
}

}  // extern "C"
