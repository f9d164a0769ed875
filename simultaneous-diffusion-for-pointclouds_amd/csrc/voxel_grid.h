// Shared declarations of the voxel-grid machinery (voxel_grid.hip): the workspace header and argument block
// of its kernels, and vox_build_cells(), the front of sdp_voxel_grid -- finite points and bounds, grid, keys,
// stable radix sort, segment heads -- which csrc/cloud_nn.hip runs on a target cloud to get its cell grid.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "radix_sort.h"

namespace sdp {

struct VoxHdr {
  float org[3];
  float pad;
  unsigned long long nx, ny;    // key = ix + nx*iy + nx*ny*iz
  long long dims[3];            // nx, ny, nz as reported (each clamped to 2^62 when the grid is too large)
  int key_bits, too_large, used, m;
  int label_bits;               // width of the (voxel row, label) keys, known once m is
  RadixState sort[2];           // [voxel keys | label keys]
  float lo[3], hi[3];           // bounds of the finite points (float32), for the consumers of the cell grid
};

struct VoxArgs {
  const float* points;
  const float* features;
  const int32_t* classes;
  int n, stride, fdim, ldim, nchunks, ntiles;
  float dl;
  float* out_points;
  float* out_features;
  int32_t* out_classes;
  int64_t* out_keys;
  int32_t* out_counts;
  int32_t* out_order;
  int32_t* out_inverse;
  int64_t* info;
  VoxHdr* hdr;
  int32_t* chunk_fin;    // [nchunks] finite points per chunk, after the scan the chunks' first rows
  float* chunk_mm;       // [nchunks][6] min xyz, max xyz of the finite points
  int32_t* chunk_head;   // [nchunks] segment heads per chunk of sorted rows, then their first voxel rows
  int32_t* tile_cnt;     // [256][ntiles] digit-major counts, after the scan the first output rows
  uint64_t* key0;
  uint64_t* key1;
  uint32_t* idx0;
  uint32_t* idx1;
  int32_t* first;        // [m] first sorted row of each voxel
  int32_t* rowof;        // [used] voxel row of each sorted row
};

// bytes of the workspace of n points (n in [1, 2^30])
size_t vox_workspace_bytes(int64_t n);
// Points a.hdr .. a.rowof, a.nchunks and a.ntiles into `workspace` and launches the stages up to the segment
// heads on `st`.  The caller has set a.points, a.n, a.stride, a.dl and whichever of a.out_keys, a.out_order and
// a.out_inverse it wants.  Afterwards, in stream order: a.hdr (used, m, org, dims, too_large, lo, hi), a.first
// [m], the sorted unique keys in a.out_keys [m] and the sorted permutation in a.out_order [used].
void vox_build_cells(VoxArgs& a, void* workspace, hipStream_t st);

}  // namespace sdp
