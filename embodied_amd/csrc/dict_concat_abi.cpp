// emb_dict_concat: nn.DictConcat (embodied/jax/nets.py:467-500) with the reset
// masks and the clamp of dreamerv3/rssm.py:76-79, 137 in one launch
// (dict_concat.hip).  Its own translation unit, as stat_rows_abi.cpp.
#include "abi_common.h"
#include "dict_concat.h"

using namespace emb_abi;

extern "C" {

int32_t emb_dict_concat(const emb_dict_entry_t* table, int64_t count, int64_t rows, int64_t width, void* out,
                        int64_t out_stride, int32_t out_dtype, const void* reset, int32_t unit, void* stream) {
  return guarded([&] {
    const char* wrong = emb::dict_concat_error(table, count, rows, width, out, out_stride, out_dtype);   // before any HIP call
    need(!wrong, wrong);
    if (rows == 0) return;
    emb::DictTable keys{};
    for (int k = 0; k < count; ++k) keys.e[k] = emb::dict_key_of(table[k]);
    HIP_OK(emb::launch_dict_concat(keys, static_cast<int>(count), rows, width, out, out_stride, out_dtype == EMB_BF16,
                                   static_cast<const uint8_t*>(reset), unit != 0, static_cast<hipStream_t>(stream)));
  });
}

int32_t emb_dict_concat_launches(int64_t* count) {
  return guarded([&] {
    need(count, "dict_concat_launches: count is null");
    *count = emb::dict_concat_launches();
  });
}

}  // extern "C"
