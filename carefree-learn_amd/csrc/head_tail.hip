// The last block of a stack whose output is read at the head token only (`net[:, 0]`) computes its projection, FF1 + GELU, FF2
// and their dX GEMMs for the B head rows alone, in place in the block's full-size [B * T, .] tensors (cfhip_gemm_bf16_rows in
// gemm.hip: M = B rows, leading dimensions T rows long, the whole launch's tile configuration).  LayerNorm, attention and the
// weight gradients stay the full-row launches they were; the rows the GEMMs skip read as zero to them.  This file holds the
// kernel that zeroes those rows.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int chunk16;  // 16 bytes: 8 bf16 or 4 f32

// the first `chunks` 16-byte pieces of `total / chunks` rows, `stride` pieces apart := 0
__global__ void head_rows_zero_kernel(chunk16* __restrict__ dst, long total, int chunks, long stride) {
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += step) {
    const long row = i / chunks;
    dst[row * stride + (i - row * chunks)] = chunk16{0u, 0u, 0u, 0u};
  }
}

}  // namespace

extern "C" int cfhip_head_rows_zero(void* dst, int rows, int cols, int64_t row_stride, int elem_bytes, void* stream) {
  CFHIP_REQUIRE(dst && rows > 0 && cols > 0 && (elem_bytes == 2 || elem_bytes == 4), "head_rows_zero: bad arguments");
  const long row_bytes = (long)cols * elem_bytes, stride_bytes = (long)row_stride * elem_bytes;
  CFHIP_REQUIRE(row_bytes % 16 == 0 && stride_bytes % 16 == 0 && stride_bytes >= row_bytes && ((uintptr_t)dst & 15) == 0,
                "head_rows_zero: rows of %ld bytes, %ld apart, must be 16-byte multiples of a 16-byte aligned tensor", row_bytes, stride_bytes);
  const int chunks = (int)(row_bytes / 16);
  const long total = (long)rows * chunks;
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(head_rows_zero_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream, (chunk16*)dst,
                     total, chunks, stride_bytes / 16);
  CFHIP_CHECK_LAUNCH("head_rows_zero");
  return CFHIP_OK;
}
