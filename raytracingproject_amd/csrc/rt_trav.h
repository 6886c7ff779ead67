// rt_trav.h -- the traversal flags of a kernel key (rt_tuning.traversal, RT_TRAV_* in
// include/rt_hip.h), for the device code (rt_device.h, which says what each flag does) and for
// the host's kernel tables and plans (rt_launch.h).  Includes nothing.
#pragma once

namespace rtx {

enum { TRAV_SELROOT = 8, TRAV_B128 = 16, TRAV_F32BOX = 32, TRAV_COH = 64, TRAV_NOSUM = 128, TRAV_TBIN = 256,
       TRAV_CULL = 512, TRAV_PERSIST = 2048, TRAV_MTOP = 4096, TRAV_MIFIF = 8192, TRAV_MWHILE = 16384,
       TRAV_MQ = 32768, TRAV_GRID = 65536, TRAV_GFLAT = 131072,
       TRAV_G3D = 262144 };
constexpr int TRAV_REMOVED = TRAV_TBIN | TRAV_MTOP;   // refused (r04)

}  // namespace rtx
