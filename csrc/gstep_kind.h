// The dtype code of a graph's global_step variable, as every kernel that bumps
// it takes it (graph_mlp.hip, ipc_coll.hip, sparse_lr.hip, mlp_persist_f32.hip).
// Host and device; GSTEP_NONE goes with a null pointer: no variable to bump.
// The host maps a tensor to (pointer, kind) in gstep_host.h.
#pragma once

namespace dtfk {

enum GstepKind : int { GSTEP_NONE = 0, GSTEP_F32 = 1, GSTEP_I64 = 2, GSTEP_I32 = 3, GSTEP_F64 = 4 };

}  // namespace dtfk
