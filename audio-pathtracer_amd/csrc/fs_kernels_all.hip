// fs_kernels_all.hip — the units fs_walk.hip, fs_connect.hip, fs_frame.hip and fs_aux_kernels.hip as ONE unit: for the
// diagnostic builds (-DFS_WAVE_TIMELINE, -DFS_TRAV_STATS; tools/build_variant.sh, the Makefile's `onefile` target), whose
// device-side debug symbols must be shared by those kernels.  The product builds every unit on its own (Makefile).
// A unit has ONE node layout (fs_dev_trav.hpp: NodeLayout), chosen when the first of these files includes the traversal:
// NodeQ4.  So the narrow flavour of THIS unit's fused frame kernel walks NodeQ4 records, bound by its own launcher to the
// NodeQ4 arrays — correct, but not the product's record format, whose narrow flavour walks the 48-byte view.  (The other
// flavours stay units of their own, as in the product.)  FS_KERNELS_ALL tells fs_frame.hip that this is intended.
#define FS_KERNELS_ALL 1
#include "fs_walk.hip"
#include "fs_connect.hip"
#include "fs_frame.hip"
#include "fs_aux_kernels.hip"
