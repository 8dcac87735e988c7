// fsmc_constants.h -- the constants that the kernels and the host's table builders (fsmc_model_tables.h) both lay
// memory out by: how wide a model each kernel family takes, the padding of a table row, the parts of a RowSet.
// Plain C++: nothing here knows the device's runtime, so the host-only headers and their CPU tests include it too.
#pragma once

namespace fsmc
{
constexpr int kMaxStates = 256; // the widest model a lane-per-pair or two-workgroups-per-CU member decodes (fsmc_instances.h)
constexpr int kMaxStatesW2 = 1024; // ... and the wave-group kernel with one workgroup per CU (four waves of 80 states, six to eight of 64;
                                    // beyond 512 states eight waves of 80 / 96 / 128 without landing zones)
constexpr int kMaxStatesAny = 4096; // ... and the any-K kernel (fsmc_kernels_any.h: K-vectors in the workspace)

constexpr int kKPad = 16;      // table / emission rows are zero padded to a multiple of this many floats
// RowSet: the transition-table rows of one key side by side, [key][5][KP] floats (packed steps)
enum RowSetPart : int { kRowD = 0, kRowB = 1, kRowU = 2, kRowUsh = 3, kRowRR = 4, kRowSetParts = 5 };
} // namespace fsmc
