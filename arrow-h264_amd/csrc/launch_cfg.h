// launch_cfg.h -- launch shapes shared by the kernels and the host (h264r_host.hip)
#pragma once

// consecutive groups (the MBs of one pass of its waves) per workgroup (k_recon.hip): k_inter4r (1: with
// more, loop-carried state spilled and config 3 lost 2 %, profiles/r03_h_inter_ab.txt; 2
// still costs config 3 4 % while config 4 gains 2 %, profiles/r03s2_s_ab.txt)
#ifndef H264R_INTER_GROUPS
#define H264R_INTER_GROUPS 1
#endif

// waves per k_inter4r workgroup, 4 or 2 (k_recon.hip): a workgroup's wave slots are released
// together, so a smaller workgroup leaves fewer of them idle behind its slowest wave (4.61 of 5
// resident per SIMD at 4; config 3 kernel_ms.inter -0.7 .. -1.5 % at 2, profiles/r12_a_inter_mc_wg_ab.txt)
#ifndef H264R_INTER_WG_WAVES
#define H264R_INTER_WG_WAVES 2
#endif
static_assert(H264R_INTER_WG_WAVES == 2 || H264R_INTER_WG_WAVES == 4, "k_inter4r: 128 or 256 threads");

// k_deblock2: MB rows per wave, walked in lock step one MB apart (k_deblock2.hip); the
// wave's 16 (picture, row) units cover 16 / H264R_DB2_BAND pictures
#ifndef H264R_DB2_BAND
#define H264R_DB2_BAND 4
#endif

// k_deblock2: lanes per (picture, MB row) unit (4 or 8); a wave holds 64 / H264R_DB2_LPU units
#ifndef H264R_DB2_LPU
#define H264R_DB2_LPU 8
#endif
