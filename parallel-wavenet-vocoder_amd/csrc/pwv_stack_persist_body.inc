// The body of the persistent flow kernels (pwv_stack_persist.hip): stack_persist_kernel<F32, MODE, VARLEN, STREAM> and
// stack_persist_ragged_kernel<F32, MODE> (VARLEN and STREAM both on) include it -- an include, not a shared __device__ function:
// a function moves the register allocation of the instantiations that exist, an include leaves their instruction streams alone
// (as pwv_layer_f16x3_body.inc between the one-shot and the streaming layer kernels).  Expects F32, MODE, VARLEN, STREAM and `p`.
// In parts, included in order (each names what it expects and what it defines):
#include "pwv_persist_geometry.inc"      // row maps, ring and P descriptors, history look-back / store, load_x / load_xc / load_xb
#include "pwv_persist_protocol.inc"      // dep_addr ... wait_deps, publish, leave_layers, task claiming
#include "pwv_persist_loader.inc"        // SHORT: the loader wave
#include "pwv_persist_fold0.inc"         // layer 0 in its folded form
#include "pwv_persist_tasks.inc"         // the task loop; the unit's arithmetic in pwv_persist_unit_f32.inc / pwv_persist_unit_f16x3.inc
#include "pwv_persist_tail.inc"          // last layer + fused head (pwv_head_*.inc) + affine
#include "pwv_persist_exit.inc"          // the last workgroup zeroes the polled words
