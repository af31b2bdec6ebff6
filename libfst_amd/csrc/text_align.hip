// text_align.hip -- the launches of the alignment kernels (kernels/text_align.hpp): input
// spans per output symbol, for fst_normalize_text_aligned_batch and the two device pieces
// fst_device_path_alignment / fst_device_compose_alignment.  DeviceEngine::align_write and
// align_compose (device_engine.hip) size the grids.
#define FSTAMD_BFS_TEMPLATES_ONLY  // device_engine.hip holds the non-template kernels
#include "device_engine.hpp"
#include "kernels/text_align.hpp"

namespace fstamd {

hipError_t launch_align_write(const BatchOutDev& s, uint32_t num, const uint64_t* offsets,
                              uint32_t* begin, uint32_t* end, uint64_t cap, uint32_t* consumed,
                              uint32_t grid, hipStream_t stream) {
  align_write_kernel<<<grid, 64, 0, stream>>>(s, num, offsets, begin, end, cap, consumed);
  return hipGetLastError();
}

hipError_t launch_align_compose(uint32_t num, const uint64_t* outer_off, const uint32_t* b,
                                const uint32_t* e, const uint64_t* inner_off,
                                const uint32_t* in_begin, const uint32_t* in_end,
                                const uint32_t* n1, uint32_t* out_begin, uint32_t* out_end,
                                uint64_t cap, uint32_t grid, hipStream_t stream) {
  align_compose_kernel<<<grid, 64, 0, stream>>>(num, outer_off, b, e, inner_off, in_begin, in_end,
                                                n1, out_begin, out_end, cap);
  return hipGetLastError();
}

}  // namespace fstamd
