// Marching cubes over a dense scalar lattice (ucsa_mc_count / ucsa_mc_emit):
// the labelled-mesh export of the semantic field (network_tcnn_semantics.py,
// extract_semantic_mesh).  Deterministic: every output slot comes from integer
// prefix sums over the point index, never from atomics, so two runs give the
// same bytes.  Conventions (include/ucsa_hip.h, utils/mc_tables.py):
//   - point (i,j,k) is field[(i*ny + j)*nz + k]; inside iff field > iso;
//   - point p owns its +x, +y, +z edges (edge id 3*p + axis); one vertex per
//     crossing edge, in ascending edge id;
//   - cell p (lower corner p) emits its TRI_TABLE row in table order; cells
//     in ascending p.
//
// Passes (tiles of MC_TILE = 1024 consecutive points, 4 per thread):
//   k_mc_classify  per point a 16-bit class (cell case | crossing edges << 8)
//                  and per tile the packed counts (vertices | triangles << 16);
//   k_mc_scan      ONE work-group: exclusive scan of the tile counts (64-bit
//                  carries), the totals; a total above 2^31-1 is reported as
//                  0xFFFFFFFF in both;
//   k_mc_offsets   per point its first vertex / triangle slot;
//   k_mc_emit      vertices (position, normal) and triangles.
// Workspace: 10 bytes per point plus 12 per tile (1.34 GB at 512^3).
//
// ucsa_mc_count_masked / ucsa_mc_emit_masked run the same kernels with a
// validity mask (uint8 per point; a TSDF volume's "observed"): an edge carries a
// vertex only between two valid points, a cell emits only with eight valid
// corners, and the normal's differences stop at an invalid neighbour.  The
// unmasked entries pass no mask and take the same path as before.
#include "ucsa_common.h"
#include "wave_ops.h"

namespace {

constexpr uint32_t MC_THREADS = 256;
constexpr uint32_t MC_ITEMS = 4;
constexpr uint32_t MC_TILE = MC_THREADS * MC_ITEMS;
constexpr uint32_t MC_SCAN_THREADS = 1024;
constexpr uint32_t MC_OVERFLOW = 0xFFFFFFFFu;

// The classic 256-case triangle table (Lorensen & Cline; the public-domain
// listing by P. Bourke).  Bit c of a case: corner c is outside (field <= iso).
// Corners 0..7 = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1)
// (0,1,1); edges 0..11 = 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7.
// Triangles as listed wind counter-clockwise seen from outside.  Constant
// memory rather than LDS: the lookups diverge per lane either way, and one
// work-group per 256 points would re-stage the 4 KB table ~500 k times at 512^3.
__constant__ int8_t kTri[256][16] = {
    {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,8,3,9,8,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,1,2,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,2,10,0,2,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,8,3,2,10,8,10,9,8,-1,-1,-1,-1,-1,-1,-1},
    {3,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,11,2,8,11,0,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,9,0,2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,11,2,1,9,11,9,8,11,-1,-1,-1,-1,-1,-1,-1},
    {3,10,1,11,10,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,10,1,0,8,10,8,11,10,-1,-1,-1,-1,-1,-1,-1},
    {3,9,0,3,11,9,11,10,9,-1,-1,-1,-1,-1,-1,-1},
    {9,8,10,10,8,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,3,0,7,3,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,8,4,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,1,9,4,7,1,7,3,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,8,4,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,4,7,3,0,4,1,2,10,-1,-1,-1,-1,-1,-1,-1},
    {9,2,10,9,0,2,8,4,7,-1,-1,-1,-1,-1,-1,-1},
    {2,10,9,2,9,7,2,7,3,7,9,4,-1,-1,-1,-1},
    {8,4,7,3,11,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,4,7,11,2,4,2,0,4,-1,-1,-1,-1,-1,-1,-1},
    {9,0,1,8,4,7,2,3,11,-1,-1,-1,-1,-1,-1,-1},
    {4,7,11,9,4,11,9,11,2,9,2,1,-1,-1,-1,-1},
    {3,10,1,3,11,10,7,8,4,-1,-1,-1,-1,-1,-1,-1},
    {1,11,10,1,4,11,1,0,4,7,11,4,-1,-1,-1,-1},
    {4,7,8,9,0,11,9,11,10,11,0,3,-1,-1,-1,-1},
    {4,7,11,4,11,9,9,11,10,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,0,8,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,5,4,1,5,0,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,5,4,8,3,5,3,1,5,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,9,5,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,0,8,1,2,10,4,9,5,-1,-1,-1,-1,-1,-1,-1},
    {5,2,10,5,4,2,4,0,2,-1,-1,-1,-1,-1,-1,-1},
    {2,10,5,3,2,5,3,5,4,3,4,8,-1,-1,-1,-1},
    {9,5,4,2,3,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,11,2,0,8,11,4,9,5,-1,-1,-1,-1,-1,-1,-1},
    {0,5,4,0,1,5,2,3,11,-1,-1,-1,-1,-1,-1,-1},
    {2,1,5,2,5,8,2,8,11,4,8,5,-1,-1,-1,-1},
    {10,3,11,10,1,3,9,5,4,-1,-1,-1,-1,-1,-1,-1},
    {4,9,5,0,8,1,8,10,1,8,11,10,-1,-1,-1,-1},
    {5,4,0,5,0,11,5,11,10,11,0,3,-1,-1,-1,-1},
    {5,4,8,5,8,10,10,8,11,-1,-1,-1,-1,-1,-1,-1},
    {9,7,8,5,7,9,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,3,0,9,5,3,5,7,3,-1,-1,-1,-1,-1,-1,-1},
    {0,7,8,0,1,7,1,5,7,-1,-1,-1,-1,-1,-1,-1},
    {1,5,3,3,5,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,7,8,9,5,7,10,1,2,-1,-1,-1,-1,-1,-1,-1},
    {10,1,2,9,5,0,5,3,0,5,7,3,-1,-1,-1,-1},
    {8,0,2,8,2,5,8,5,7,10,5,2,-1,-1,-1,-1},
    {2,10,5,2,5,3,3,5,7,-1,-1,-1,-1,-1,-1,-1},
    {7,9,5,7,8,9,3,11,2,-1,-1,-1,-1,-1,-1,-1},
    {9,5,7,9,7,2,9,2,0,2,7,11,-1,-1,-1,-1},
    {2,3,11,0,1,8,1,7,8,1,5,7,-1,-1,-1,-1},
    {11,2,1,11,1,7,7,1,5,-1,-1,-1,-1,-1,-1,-1},
    {9,5,8,8,5,7,10,1,3,10,3,11,-1,-1,-1,-1},
    {5,7,0,5,0,9,7,11,0,1,0,10,11,10,0,-1},
    {11,10,0,11,0,3,10,5,0,8,0,7,5,7,0,-1},
    {11,10,5,7,11,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {10,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,0,1,5,10,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,8,3,1,9,8,5,10,6,-1,-1,-1,-1,-1,-1,-1},
    {1,6,5,2,6,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,6,5,1,2,6,3,0,8,-1,-1,-1,-1,-1,-1,-1},
    {9,6,5,9,0,6,0,2,6,-1,-1,-1,-1,-1,-1,-1},
    {5,9,8,5,8,2,5,2,6,3,2,8,-1,-1,-1,-1},
    {2,3,11,10,6,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,0,8,11,2,0,10,6,5,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,2,3,11,5,10,6,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,1,9,2,9,11,2,9,8,11,-1,-1,-1,-1},
    {6,3,11,6,5,3,5,1,3,-1,-1,-1,-1,-1,-1,-1},
    {0,8,11,0,11,5,0,5,1,5,11,6,-1,-1,-1,-1},
    {3,11,6,0,3,6,0,6,5,0,5,9,-1,-1,-1,-1},
    {6,5,9,6,9,11,11,9,8,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,4,7,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,3,0,4,7,3,6,5,10,-1,-1,-1,-1,-1,-1,-1},
    {1,9,0,5,10,6,8,4,7,-1,-1,-1,-1,-1,-1,-1},
    {10,6,5,1,9,7,1,7,3,7,9,4,-1,-1,-1,-1},
    {6,1,2,6,5,1,4,7,8,-1,-1,-1,-1,-1,-1,-1},
    {1,2,5,5,2,6,3,0,4,3,4,7,-1,-1,-1,-1},
    {8,4,7,9,0,5,0,6,5,0,2,6,-1,-1,-1,-1},
    {7,3,9,7,9,4,3,2,9,5,9,6,2,6,9,-1},
    {3,11,2,7,8,4,10,6,5,-1,-1,-1,-1,-1,-1,-1},
    {5,10,6,4,7,2,4,2,0,2,7,11,-1,-1,-1,-1},
    {0,1,9,4,7,8,2,3,11,5,10,6,-1,-1,-1,-1},
    {9,2,1,9,11,2,9,4,11,7,11,4,5,10,6,-1},
    {8,4,7,3,11,5,3,5,1,5,11,6,-1,-1,-1,-1},
    {5,1,11,5,11,6,1,0,11,7,11,4,0,4,11,-1},
    {0,5,9,0,6,5,0,3,6,11,6,3,8,4,7,-1},
    {6,5,9,6,9,11,4,7,9,7,11,9,-1,-1,-1,-1},
    {10,4,9,6,4,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,10,6,4,9,10,0,8,3,-1,-1,-1,-1,-1,-1,-1},
    {10,0,1,10,6,0,6,4,0,-1,-1,-1,-1,-1,-1,-1},
    {8,3,1,8,1,6,8,6,4,6,1,10,-1,-1,-1,-1},
    {1,4,9,1,2,4,2,6,4,-1,-1,-1,-1,-1,-1,-1},
    {3,0,8,1,2,9,2,4,9,2,6,4,-1,-1,-1,-1},
    {0,2,4,4,2,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,3,2,8,2,4,4,2,6,-1,-1,-1,-1,-1,-1,-1},
    {10,4,9,10,6,4,11,2,3,-1,-1,-1,-1,-1,-1,-1},
    {0,8,2,2,8,11,4,9,10,4,10,6,-1,-1,-1,-1},
    {3,11,2,0,1,6,0,6,4,6,1,10,-1,-1,-1,-1},
    {6,4,1,6,1,10,4,8,1,2,1,11,8,11,1,-1},
    {9,6,4,9,3,6,9,1,3,11,6,3,-1,-1,-1,-1},
    {8,11,1,8,1,0,11,6,1,9,1,4,6,4,1,-1},
    {3,11,6,3,6,0,0,6,4,-1,-1,-1,-1,-1,-1,-1},
    {6,4,8,11,6,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,10,6,7,8,10,8,9,10,-1,-1,-1,-1,-1,-1,-1},
    {0,7,3,0,10,7,0,9,10,6,7,10,-1,-1,-1,-1},
    {10,6,7,1,10,7,1,7,8,1,8,0,-1,-1,-1,-1},
    {10,6,7,10,7,1,1,7,3,-1,-1,-1,-1,-1,-1,-1},
    {1,2,6,1,6,8,1,8,9,8,6,7,-1,-1,-1,-1},
    {2,6,9,2,9,1,6,7,9,0,9,3,7,3,9,-1},
    {7,8,0,7,0,6,6,0,2,-1,-1,-1,-1,-1,-1,-1},
    {7,3,2,6,7,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,11,10,6,8,10,8,9,8,6,7,-1,-1,-1,-1},
    {2,0,7,2,7,11,0,9,7,6,7,10,9,10,7,-1},
    {1,8,0,1,7,8,1,10,7,6,7,10,2,3,11,-1},
    {11,2,1,11,1,7,10,6,1,6,7,1,-1,-1,-1,-1},
    {8,9,6,8,6,7,9,1,6,11,6,3,1,3,6,-1},
    {0,9,1,11,6,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,8,0,7,0,6,3,11,0,11,6,0,-1,-1,-1,-1},
    {7,11,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,6,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,0,8,11,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,1,9,11,7,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,1,9,8,3,1,11,7,6,-1,-1,-1,-1,-1,-1,-1},
    {10,1,2,6,11,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,3,0,8,6,11,7,-1,-1,-1,-1,-1,-1,-1},
    {2,9,0,2,10,9,6,11,7,-1,-1,-1,-1,-1,-1,-1},
    {6,11,7,2,10,3,10,8,3,10,9,8,-1,-1,-1,-1},
    {7,2,3,6,2,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {7,0,8,7,6,0,6,2,0,-1,-1,-1,-1,-1,-1,-1},
    {2,7,6,2,3,7,0,1,9,-1,-1,-1,-1,-1,-1,-1},
    {1,6,2,1,8,6,1,9,8,8,7,6,-1,-1,-1,-1},
    {10,7,6,10,1,7,1,3,7,-1,-1,-1,-1,-1,-1,-1},
    {10,7,6,1,7,10,1,8,7,1,0,8,-1,-1,-1,-1},
    {0,3,7,0,7,10,0,10,9,6,10,7,-1,-1,-1,-1},
    {7,6,10,7,10,8,8,10,9,-1,-1,-1,-1,-1,-1,-1},
    {6,8,4,11,8,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,6,11,3,0,6,0,4,6,-1,-1,-1,-1,-1,-1,-1},
    {8,6,11,8,4,6,9,0,1,-1,-1,-1,-1,-1,-1,-1},
    {9,4,6,9,6,3,9,3,1,11,3,6,-1,-1,-1,-1},
    {6,8,4,6,11,8,2,10,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,3,0,11,0,6,11,0,4,6,-1,-1,-1,-1},
    {4,11,8,4,6,11,0,2,9,2,10,9,-1,-1,-1,-1},
    {10,9,3,10,3,2,9,4,3,11,3,6,4,6,3,-1},
    {8,2,3,8,4,2,4,6,2,-1,-1,-1,-1,-1,-1,-1},
    {0,4,2,4,6,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,9,0,2,3,4,2,4,6,4,3,8,-1,-1,-1,-1},
    {1,9,4,1,4,2,2,4,6,-1,-1,-1,-1,-1,-1,-1},
    {8,1,3,8,6,1,8,4,6,6,10,1,-1,-1,-1,-1},
    {10,1,0,10,0,6,6,0,4,-1,-1,-1,-1,-1,-1,-1},
    {4,6,3,4,3,8,6,10,3,0,3,9,10,9,3,-1},
    {10,9,4,6,10,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,9,5,7,6,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,4,9,5,11,7,6,-1,-1,-1,-1,-1,-1,-1},
    {5,0,1,5,4,0,7,6,11,-1,-1,-1,-1,-1,-1,-1},
    {11,7,6,8,3,4,3,5,4,3,1,5,-1,-1,-1,-1},
    {9,5,4,10,1,2,7,6,11,-1,-1,-1,-1,-1,-1,-1},
    {6,11,7,1,2,10,0,8,3,4,9,5,-1,-1,-1,-1},
    {7,6,11,5,4,10,4,2,10,4,0,2,-1,-1,-1,-1},
    {3,4,8,3,5,4,3,2,5,10,5,2,11,7,6,-1},
    {7,2,3,7,6,2,5,4,9,-1,-1,-1,-1,-1,-1,-1},
    {9,5,4,0,8,6,0,6,2,6,8,7,-1,-1,-1,-1},
    {3,6,2,3,7,6,1,5,0,5,4,0,-1,-1,-1,-1},
    {6,2,8,6,8,7,2,1,8,4,8,5,1,5,8,-1},
    {9,5,4,10,1,6,1,7,6,1,3,7,-1,-1,-1,-1},
    {1,6,10,1,7,6,1,0,7,8,7,0,9,5,4,-1},
    {4,0,10,4,10,5,0,3,10,6,10,7,3,7,10,-1},
    {7,6,10,7,10,8,5,4,10,4,8,10,-1,-1,-1,-1},
    {6,9,5,6,11,9,11,8,9,-1,-1,-1,-1,-1,-1,-1},
    {3,6,11,0,6,3,0,5,6,0,9,5,-1,-1,-1,-1},
    {0,11,8,0,5,11,0,1,5,5,6,11,-1,-1,-1,-1},
    {6,11,3,6,3,5,5,3,1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,10,9,5,11,9,11,8,11,5,6,-1,-1,-1,-1},
    {0,11,3,0,6,11,0,9,6,5,6,9,1,2,10,-1},
    {11,8,5,11,5,6,8,0,5,10,5,2,0,2,5,-1},
    {6,11,3,6,3,5,2,10,3,10,5,3,-1,-1,-1,-1},
    {5,8,9,5,2,8,5,6,2,3,8,2,-1,-1,-1,-1},
    {9,5,6,9,6,0,0,6,2,-1,-1,-1,-1,-1,-1,-1},
    {1,5,8,1,8,0,5,6,8,3,8,2,6,2,8,-1},
    {1,5,6,2,1,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,3,6,1,6,10,3,8,6,5,6,9,8,9,6,-1},
    {10,1,0,10,0,6,9,5,0,5,6,0,-1,-1,-1,-1},
    {0,3,8,5,6,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {10,5,6,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,5,10,7,5,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {11,5,10,11,7,5,8,3,0,-1,-1,-1,-1,-1,-1,-1},
    {5,11,7,5,10,11,1,9,0,-1,-1,-1,-1,-1,-1,-1},
    {10,7,5,10,11,7,9,8,1,8,3,1,-1,-1,-1,-1},
    {11,1,2,11,7,1,7,5,1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,1,2,7,1,7,5,7,2,11,-1,-1,-1,-1},
    {9,7,5,9,2,7,9,0,2,2,11,7,-1,-1,-1,-1},
    {7,5,2,7,2,11,5,9,2,3,2,8,9,8,2,-1},
    {2,5,10,2,3,5,3,7,5,-1,-1,-1,-1,-1,-1,-1},
    {8,2,0,8,5,2,8,7,5,10,2,5,-1,-1,-1,-1},
    {9,0,1,5,10,3,5,3,7,3,10,2,-1,-1,-1,-1},
    {9,8,2,9,2,1,8,7,2,10,2,5,7,5,2,-1},
    {1,3,5,3,7,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,8,7,0,7,1,1,7,5,-1,-1,-1,-1,-1,-1,-1},
    {9,0,3,9,3,5,5,3,7,-1,-1,-1,-1,-1,-1,-1},
    {9,8,7,5,9,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {5,8,4,5,10,8,10,11,8,-1,-1,-1,-1,-1,-1,-1},
    {5,0,4,5,11,0,5,10,11,11,3,0,-1,-1,-1,-1},
    {0,1,9,8,4,10,8,10,11,10,4,5,-1,-1,-1,-1},
    {10,11,4,10,4,5,11,3,4,9,4,1,3,1,4,-1},
    {2,5,1,2,8,5,2,11,8,4,5,8,-1,-1,-1,-1},
    {0,4,11,0,11,3,4,5,11,2,11,1,5,1,11,-1},
    {0,2,5,0,5,9,2,11,5,4,5,8,11,8,5,-1},
    {9,4,5,2,11,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,5,10,3,5,2,3,4,5,3,8,4,-1,-1,-1,-1},
    {5,10,2,5,2,4,4,2,0,-1,-1,-1,-1,-1,-1,-1},
    {3,10,2,3,5,10,3,8,5,4,5,8,0,1,9,-1},
    {5,10,2,5,2,4,1,9,2,9,4,2,-1,-1,-1,-1},
    {8,4,5,8,5,3,3,5,1,-1,-1,-1,-1,-1,-1,-1},
    {0,4,5,1,0,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {8,4,5,8,5,3,9,0,5,0,3,5,-1,-1,-1,-1},
    {9,4,5,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,11,7,4,9,11,9,10,11,-1,-1,-1,-1,-1,-1,-1},
    {0,8,3,4,9,7,9,11,7,9,10,11,-1,-1,-1,-1},
    {1,10,11,1,11,4,1,4,0,7,4,11,-1,-1,-1,-1},
    {3,1,4,3,4,8,1,10,4,7,4,11,10,11,4,-1},
    {4,11,7,9,11,4,9,2,11,9,1,2,-1,-1,-1,-1},
    {9,7,4,9,11,7,9,1,11,2,11,1,0,8,3,-1},
    {11,7,4,11,4,2,2,4,0,-1,-1,-1,-1,-1,-1,-1},
    {11,7,4,11,4,2,8,3,4,3,2,4,-1,-1,-1,-1},
    {2,9,10,2,7,9,2,3,7,7,4,9,-1,-1,-1,-1},
    {9,10,7,9,7,4,10,2,7,8,7,0,2,0,7,-1},
    {3,7,10,3,10,2,7,4,10,1,10,0,4,0,10,-1},
    {1,10,2,8,7,4,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,9,1,4,1,7,7,1,3,-1,-1,-1,-1,-1,-1,-1},
    {4,9,1,4,1,7,0,8,1,8,7,1,-1,-1,-1,-1},
    {4,0,3,7,4,3,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {4,8,7,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {9,10,8,10,11,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,0,9,3,9,11,11,9,10,-1,-1,-1,-1,-1,-1,-1},
    {0,1,10,0,10,8,8,10,11,-1,-1,-1,-1,-1,-1,-1},
    {3,1,10,11,3,10,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,2,11,1,11,9,9,11,8,-1,-1,-1,-1,-1,-1,-1},
    {3,0,9,3,9,11,1,2,9,2,11,9,-1,-1,-1,-1},
    {0,2,11,8,0,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {3,2,11,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,8,2,8,10,10,8,9,-1,-1,-1,-1,-1,-1,-1},
    {9,10,2,0,9,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {2,3,8,2,8,10,0,1,8,1,10,8,-1,-1,-1,-1},
    {1,10,2,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {1,3,8,9,1,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,9,1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {0,3,8,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},
    {-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1},};

// cube edge e: owner point offset (di, dj, dk) and axis, packed as
// di | dj << 1 | dk << 2 | axis << 3 (utils/mc_tables.py EDGE_OWNER)
__constant__ uint8_t kEdgeOwner[12] = {
    0 | 0 << 3, 1 | 1 << 3, 2 | 0 << 3, 0 | 1 << 3,
    4 | 0 << 3, 5 | 1 << 3, 6 | 0 << 3, 4 | 1 << 3,
    0 | 2 << 3, 1 | 2 << 3, 3 | 2 << 3, 2 | 2 << 3};

struct McDims {
  uint32_t nx, ny, nz, n;  // n = nx*ny*nz points (< 2^31)
};

__device__ __forceinline__ uint32_t mc_ntri(uint32_t c) {
  uint32_t t = 0;
  while (t < 5 && kTri[c][3 * t] >= 0) ++t;
  return t;
}

__device__ __forceinline__ bool mc_out(const float* f, uint32_t q, float iso) {
  return !(f[q] > iso);  // NaN counts as outside
}

// class of point p: cell case (0 where p is no cell's lower corner) | crossing
// edges << 8
__device__ uint32_t mc_class(const float* __restrict__ f,
                             const uint8_t* __restrict__ valid, McDims d, float iso,
                             uint32_t p) {
  const uint32_t sy = d.nz, sx = d.ny * d.nz;
  const uint32_t k = p % d.nz, r = p / d.nz, j = r % d.ny, i = r / d.ny;
  const bool hx = i + 1 < d.nx, hy = j + 1 < d.ny, hz = k + 1 < d.nz;
  const bool o0 = mc_out(f, p, iso);
  uint32_t e = 0;
  if (hx && mc_out(f, p + sx, iso) != o0) e |= 1u;
  if (hy && mc_out(f, p + sy, iso) != o0) e |= 2u;
  if (hz && mc_out(f, p + 1, iso) != o0) e |= 4u;
  uint32_t c = 0;
  if (hx && hy && hz) {
    c = (uint32_t)o0 | (uint32_t)mc_out(f, p + sx, iso) << 1 |
        (uint32_t)mc_out(f, p + sx + sy, iso) << 2 |
        (uint32_t)mc_out(f, p + sy, iso) << 3 | (uint32_t)mc_out(f, p + 1, iso) << 4 |
        (uint32_t)mc_out(f, p + sx + 1, iso) << 5 |
        (uint32_t)mc_out(f, p + sx + sy + 1, iso) << 6 |
        (uint32_t)mc_out(f, p + sy + 1, iso) << 7;
  }
  if (valid) {
    // an edge needs both end points, a cell all eight corners
    const bool v0 = valid[p] != 0;
    const bool vx = hx && valid[p + sx], vy = hy && valid[p + sy], vz = hz && valid[p + 1];
    e &= v0 ? ((uint32_t)vx | (uint32_t)vy << 1 | (uint32_t)vz << 2) : 0u;
    if (c && !(v0 && vx && vy && vz && valid[p + sx + sy] && valid[p + sx + 1] &&
               valid[p + sx + sy + 1] && valid[p + sy + 1]))
      c = 0;
  }
  return c | e << 8;
}

// vertices | triangles << 16 of one class
__device__ __forceinline__ uint32_t mc_counts(uint32_t cls) {
  return (uint32_t)__popc(cls >> 8) | mc_ntri(cls & 255u) << 16;
}

// exclusive scan over a MC_THREADS work-group; *total = the group's sum
__device__ __forceinline__ uint32_t mc_block_excl(uint32_t v, uint32_t* lds,
                                                  uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan_add_u32(v, lane);
  if (lane == 63) lds[w] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t q = 0; q < MC_THREADS / 64; ++q) {
    const uint32_t x = lds[q];
    if (q < w) base += x;
    tot += x;
  }
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_classify(
    const float* __restrict__ f, const uint8_t* __restrict__ valid, McDims d, float iso,
    uint16_t* __restrict__ cls, uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t lds[MC_THREADS / 64];
  const uint32_t p0 = blockIdx.x * MC_TILE + threadIdx.x * MC_ITEMS;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t q = 0; q < MC_ITEMS; ++q) {
    const uint32_t p = p0 + q;
    if (p < d.n) {
      const uint32_t c = mc_class(f, valid, d, iso, p);
      cls[p] = (uint16_t)c;
      sum += mc_counts(c);
    }
  }
  uint32_t total;
  mc_block_excl(sum, lds, &total);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one work-group: tile_counts -> exclusive tile offsets; totals[0] = V, [1] = F
__global__ __launch_bounds__(MC_SCAN_THREADS) void k_mc_scan(
    const uint32_t* __restrict__ tile_counts, uint32_t n_tiles,
    uint32_t* __restrict__ tile_v, uint32_t* __restrict__ tile_f,
    uint32_t* __restrict__ totals) {
  __shared__ uint32_t lds_v[MC_SCAN_THREADS / 64], lds_f[MC_SCAN_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t carry_v = 0, carry_f = 0;
  for (uint32_t b0 = 0; b0 < n_tiles; b0 += MC_SCAN_THREADS) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t c = b < n_tiles ? tile_counts[b] : 0u;
    const uint32_t v = c & 0xFFFFu, fc = c >> 16;
    const uint32_t iv = wave_incl_scan_add_u32(v, lane);
    const uint32_t jf = wave_incl_scan_add_u32(fc, lane);
    if (lane == 63) {
      lds_v[w] = iv;
      lds_f[w] = jf;
    }
    __syncthreads();
    uint32_t bv = 0, bf = 0, tv = 0, tf = 0;
    for (uint32_t q = 0; q < MC_SCAN_THREADS / 64; ++q) {
      const uint32_t xv = lds_v[q], xf = lds_f[q];
      if (q < w) {
        bv += xv;
        bf += xf;
      }
      tv += xv;
      tf += xf;
    }
    if (b < n_tiles) {
      // offsets wrap above 2^32 only after the totals have overflowed, and the
      // overflow sentinel then forbids the emit pass
      tile_v[b] = (uint32_t)(carry_v + bv + iv - v);
      tile_f[b] = (uint32_t)(carry_f + bf + jf - fc);
    }
    carry_v += tv;
    carry_f += tf;
    __syncthreads();  // lds reused by the next chunk
  }
  if (threadIdx.x == 0) {
    const bool over = carry_v > 0x7FFFFFFFull || carry_f > 0x7FFFFFFFull;
    totals[0] = over ? MC_OVERFLOW : (uint32_t)carry_v;
    totals[1] = over ? MC_OVERFLOW : (uint32_t)carry_f;
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_offsets(
    const uint16_t* __restrict__ cls, McDims d, const uint32_t* __restrict__ tile_v,
    const uint32_t* __restrict__ tile_f, uint32_t* __restrict__ voff,
    uint32_t* __restrict__ foff) {
  __shared__ uint32_t lds[MC_THREADS / 64];
  const uint32_t p0 = blockIdx.x * MC_TILE + threadIdx.x * MC_ITEMS;
  uint32_t cnt[MC_ITEMS];
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t q = 0; q < MC_ITEMS; ++q) {
    const uint32_t p = p0 + q;
    cnt[q] = p < d.n ? mc_counts(cls[p]) : 0u;
    sum += cnt[q];
  }
  uint32_t total;
  const uint32_t ex = mc_block_excl(sum, lds, &total);
  uint32_t v = tile_v[blockIdx.x] + (ex & 0xFFFFu);
  uint32_t t = tile_f[blockIdx.x] + (ex >> 16);
#pragma unroll
  for (uint32_t q = 0; q < MC_ITEMS; ++q) {
    const uint32_t p = p0 + q;
    if (p < d.n) {
      voff[p] = v;
      foff[p] = t;
    }
    v += cnt[q] & 0xFFFFu;
    t += cnt[q] >> 16;
  }
}

// -grad f at lattice point q (index idx along `axis`, stride s, n points):
// central difference inside, one-sided on the boundary and next to an invalid
// neighbour; +0 when neither neighbour can be used
__device__ __forceinline__ float mc_neg_grad(const float* __restrict__ f,
                                             const uint8_t* __restrict__ valid, uint32_t q,
                                             uint32_t idx, uint32_t n, uint32_t s,
                                             float h) {
  uint32_t hi = idx + 1 < n ? idx + 1 : idx;
  uint32_t lo = idx > 0 ? idx - 1 : idx;
  if (valid) {
    if (!valid[q + (hi - idx) * s]) hi = idx;
    if (!valid[q - (idx - lo) * s]) lo = idx;
    if (hi == lo) return 0.0f;
  }
  const float df = f[q + (hi - idx) * s] - f[q - (idx - lo) * s];
  const float den = (float)(hi - lo) * h;
  return -(df / den);
}

struct McFrame {
  float o[3], h[3];
};

__global__ __launch_bounds__(MC_THREADS) void k_mc_emit(
    const float* __restrict__ f, const uint8_t* __restrict__ valid, McDims d, float iso,
    McFrame fr, const uint16_t* __restrict__ cls, const uint32_t* __restrict__ voff,
    const uint32_t* __restrict__ foff, float* __restrict__ verts,
    float* __restrict__ normals, int32_t* __restrict__ tris, uint32_t max_verts,
    uint32_t max_faces) {
  const uint32_t p = blockIdx.x * MC_THREADS + threadIdx.x;
  if (p >= d.n) return;
  const uint32_t c = cls[p];
  const uint32_t edges = c >> 8, cs = c & 255u;
  if (edges == 0 && cs == 0) return;
  const uint32_t sy = d.nz, sx = d.ny * d.nz;
  const uint32_t k = p % d.nz, r = p / d.nz, j = r % d.ny, i = r / d.ny;
  const uint32_t ijk[3] = {i, j, k}, dim[3] = {d.nx, d.ny, d.nz}, st[3] = {sx, sy, 1u};
  uint32_t v = voff[p];
  for (uint32_t a = 0; a < 3; ++a) {
    if (!((edges >> a) & 1u)) continue;
    if (v < max_verts) {
      const uint32_t p1 = p + st[a];
      const float f0 = f[p], f1 = f[p1];
      const float t = (iso - f0) / (f1 - f0);
      float x[3], g0[3], g1[3];
      for (uint32_t b = 0; b < 3; ++b) x[b] = fr.o[b] + (float)ijk[b] * fr.h[b];
      x[a] = x[a] + t * fr.h[a];
      for (uint32_t b = 0; b < 3; ++b) {
        const uint32_t i1 = ijk[b] + (b == a ? 1u : 0u);
        g0[b] = mc_neg_grad(f, valid, p, ijk[b], dim[b], st[b], fr.h[b]);
        g1[b] = mc_neg_grad(f, valid, p1, i1, dim[b], st[b], fr.h[b]);
      }
      float n[3];
      for (uint32_t b = 0; b < 3; ++b) n[b] = g0[b] + t * (g1[b] - g0[b]);
      const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      for (uint32_t b = 0; b < 3; ++b) {
        verts[3ull * v + b] = x[b];
        normals[3ull * v + b] = len > 0.0f ? n[b] / len : 0.0f;
      }
    }
    ++v;
  }
  if (cs == 0) return;
  uint32_t t = foff[p];
  for (uint32_t s = 0; s < 5 && kTri[cs][3 * s] >= 0; ++s, ++t) {
    if (t >= max_faces) break;
    for (uint32_t m = 0; m < 3; ++m) {
      const uint32_t o = kEdgeOwner[kTri[cs][3 * s + m]];
      const uint32_t q = p + (o & 1u) * sx + ((o >> 1) & 1u) * sy + ((o >> 2) & 1u);
      const uint32_t a = o >> 3;
      const uint32_t below = ((uint32_t)cls[q] >> 8) & ((1u << a) - 1u);
      tris[3ull * t + m] = (int32_t)(voff[q] + (uint32_t)__popc(below));
    }
  }
}

struct McLayout {
  uint64_t cls, voff, foff, tiles, tile_v, tile_f, total;
};

McLayout mc_layout(uint64_t n) {
  auto up = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
  const uint64_t n_tiles = (n + MC_TILE - 1) / MC_TILE;
  McLayout l;
  l.cls = 0;
  l.voff = l.cls + up(2 * n);
  l.foff = l.voff + up(4 * n);
  l.tiles = l.foff + up(4 * n);
  l.tile_v = l.tiles + up(4 * n_tiles);
  l.tile_f = l.tile_v + up(4 * n_tiles);
  l.total = l.tile_f + up(4 * n_tiles);
  return l;
}

bool mc_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
  return (uint64_t)nx * ny * nz <= 0x7FFFFFFFull;
}

}  // namespace

extern "C" uint64_t ucsa_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
  return mc_layout((uint64_t)nx * ny * nz).total;
}

// k0: the argument index of nx (0-based) in the calling entry
static int32_t mc_count(const float* field, const uint8_t* valid, int k0, uint32_t nx,
                        uint32_t ny, uint32_t nz, float iso, void* workspace,
                        uint32_t* totals_dev, void* stream) {
  UCSA_CHECK_ARG(field, 0);
  UCSA_CHECK_ARG(nx >= 2 && mc_dims_ok(nx, ny, nz), k0);
  UCSA_CHECK_ARG(ny >= 2, k0 + 1);
  UCSA_CHECK_ARG(nz >= 2, k0 + 2);
  UCSA_CHECK_ARG(workspace, k0 + 4);
  UCSA_CHECK_ARG(totals_dev, k0 + 5);
  const McDims d{nx, ny, nz, nx * ny * nz};
  const McLayout l = mc_layout(d.n);
  char* ws = (char*)workspace;
  const uint32_t n_tiles = ucsa_div_up(d.n, MC_TILE);
  hipStream_t s = (hipStream_t)stream;
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_mc_classify, dim3(n_tiles), dim3(MC_THREADS), 0, s, field,
                     valid, d, iso, (uint16_t*)(ws + l.cls), (uint32_t*)(ws + l.tiles));
  hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, s,
                     (const uint32_t*)(ws + l.tiles), n_tiles,
                     (uint32_t*)(ws + l.tile_v), (uint32_t*)(ws + l.tile_f), totals_dev);
  hipLaunchKernelGGL(k_mc_offsets, dim3(n_tiles), dim3(MC_THREADS), 0, s,
                     (const uint16_t*)(ws + l.cls), d, (const uint32_t*)(ws + l.tile_v),
                     (const uint32_t*)(ws + l.tile_f), (uint32_t*)(ws + l.voff),
                     (uint32_t*)(ws + l.foff));
  return ucsa_launch_status();
}

static int32_t mc_emit(const float* field, const uint8_t* valid, int k0, uint32_t nx,
                       uint32_t ny, uint32_t nz, float iso, const float* origin3,
                       const float* spacing3, const void* workspace, float* verts,
                       float* normals, int32_t* tris, uint32_t max_verts,
                       uint32_t max_faces, void* stream) {
  UCSA_CHECK_ARG(field, 0);
  UCSA_CHECK_ARG(nx >= 2 && mc_dims_ok(nx, ny, nz), k0);
  UCSA_CHECK_ARG(ny >= 2, k0 + 1);
  UCSA_CHECK_ARG(nz >= 2, k0 + 2);
  UCSA_CHECK_ARG(origin3, k0 + 4);
  UCSA_CHECK_ARG(spacing3, k0 + 5);
  UCSA_CHECK_ARG(workspace, k0 + 6);
  UCSA_CHECK_ARG(verts || max_verts == 0, k0 + 7);
  UCSA_CHECK_ARG(normals || max_verts == 0, k0 + 8);
  UCSA_CHECK_ARG(tris || max_faces == 0, k0 + 9);
  if (max_verts == 0 && max_faces == 0) return 0;
  const McDims d{nx, ny, nz, nx * ny * nz};
  const McLayout l = mc_layout(d.n);
  const char* ws = (const char*)workspace;
  McFrame fr;
  for (int b = 0; b < 3; ++b) {
    fr.o[b] = origin3[b];
    fr.h[b] = spacing3[b];
  }
  UCSA_CLEAR_ERR();
  hipLaunchKernelGGL(k_mc_emit, dim3(ucsa_div_up(d.n, MC_THREADS)), dim3(MC_THREADS), 0,
                     (hipStream_t)stream, field, valid, d, iso, fr, (const uint16_t*)(ws + l.cls),
                     (const uint32_t*)(ws + l.voff), (const uint32_t*)(ws + l.foff), verts,
                     normals, tris, max_verts, max_faces);
  return ucsa_launch_status();
}

extern "C" int32_t ucsa_mc_count(const float* field, uint32_t nx, uint32_t ny,
                                 uint32_t nz, float iso, void* workspace,
                                 uint32_t* totals_dev, void* stream) {
  return mc_count(field, nullptr, 1, nx, ny, nz, iso, workspace, totals_dev, stream);
}

extern "C" int32_t ucsa_mc_emit(const float* field, uint32_t nx, uint32_t ny,
                                uint32_t nz, float iso, const float* origin3,
                                const float* spacing3, const void* workspace,
                                float* verts, float* normals, int32_t* tris,
                                uint32_t max_verts, uint32_t max_faces, void* stream) {
  return mc_emit(field, nullptr, 1, nx, ny, nz, iso, origin3, spacing3, workspace, verts,
                 normals, tris, max_verts, max_faces, stream);
}

extern "C" int32_t ucsa_mc_count_masked(const float* field, const uint8_t* valid,
                                        uint32_t nx, uint32_t ny, uint32_t nz, float iso,
                                        void* workspace, uint32_t* totals_dev,
                                        void* stream) {
  UCSA_CHECK_ARG(valid, 1);
  return mc_count(field, valid, 2, nx, ny, nz, iso, workspace, totals_dev, stream);
}

extern "C" int32_t ucsa_mc_emit_masked(const float* field, const uint8_t* valid,
                                       uint32_t nx, uint32_t ny, uint32_t nz, float iso,
                                       const float* origin3, const float* spacing3,
                                       const void* workspace, float* verts, float* normals,
                                       int32_t* tris, uint32_t max_verts,
                                       uint32_t max_faces, void* stream) {
  UCSA_CHECK_ARG(valid, 1);
  return mc_emit(field, valid, 2, nx, ny, nz, iso, origin3, spacing3, workspace, verts,
                 normals, tris, max_verts, max_faces, stream);
}
