// nca_step.hip -- the build unit of the fused per-step kernels.  The sources are split by kernel family:
//   nca_dynca_fwd.hip      forward launchers of the DyNCA step           (kernel, variants, launcher, ladder: nca_dynca_step.h)
//   nca_dynca_bwd.hip      backward launchers of the DyNCA step and its stencil-adjoint kernels
//   nca_cond_generic.hip   the generic ConditionedNCA step kernel and the ConditionedNCA step dispatch
// Each of them compiles on its own, but they are compiled HERE, as one unit, on purpose.  The staging helpers of nca_step_tile.h are
// internal functions that both step kernels call, and the optimiser specialises such a function, before it is inlined, on whatever
// ALL its callers in the unit agree on: TilePos::init's pad mode is a constant in the ConditionedNCA kernel only, pos_load's `sub` is
// zero in every DyNCA call but not in the ConditionedNCA kernel's goal load.  Compiled apart, 94 of the 108 kernels come out with a
// different instruction stream (same registers, LDS and occupancy).  Listing the three files in the Makefile INSTEAD of this one
// (never beside it) is all it takes to split the unit -- together with a measurement of every kernel it changes.
// To reproduce: compile this unit and the three files with `hipcc $(CXXFLAGS) --cuda-device-only -S`, then
//   python tools/isa_compare.py nca_step.s -- nca_cond_generic.s nca_dynca_fwd.s nca_dynca_bwd.s
#include "nca_cond_generic.hip"
#include "nca_dynca_fwd.hip"
#include "nca_dynca_bwd.hip"
