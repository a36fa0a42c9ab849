// Layout of the E tables (E_00 = B0^T W B0, E_11 = B1^T W B1, 12 x 12 each) in LDS, stages 1-2 of the solve kernels.
//
// Stage 2 reads E[u][v] with the ROW u = 3 foot + axis per lane and the column the same over a wave (64-row classes), so the
// lanes of an LDS lane group hold up to twelve different rows.  Two tables of 12 x 12 doubles (row stride 24 dwords) put rows
// u, u + 4, u + 8 on the same banks: a three-way conflict in every group of a two-address 8-byte load (32 banks).
//
// Here the two tables are INTERLEAVED, entry (u, v) = the 16-byte pair (E_00[u][v], E_11[u][v]) that stage 2 always uses
// together, fetched by one 16-byte load (64 banks), and a row is PADDED to 13 pairs = 52 dwords: 52 u mod 64 for u = 0 .. 11 is
// {0, 52, 40, 28, 16, 4, 56, 44, 32, 20, 8, 60}, twelve disjoint runs of four banks.  Any map of lanes to rows is free of
// conflicts at a wave-uniform column.  (tests/test_etab_layout_cpu.py replays the bank rules on this formula.)
//
// Host-compilable: no HIP in here.
#pragma once

#define QMPC_E_DIM 12        // rows and columns of a table
#define QMPC_E_ROW_PAIRS 13  // pairs per padded row
#define QMPC_E_PAIRS (QMPC_E_DIM * QMPC_E_ROW_PAIRS)  // pairs of storage (the last row's padding included)
#define QMPC_E_PAIR_BYTES 16

// offset of the pair (E_00[u][v], E_11[u][v]), in pairs (16 bytes each) from the 16-byte aligned base
constexpr int qmpc_e_pair(int u, int v) { return u * QMPC_E_ROW_PAIRS + v; }

// the layout this one replaced, kept for the bank-rule test: offset of E[u][v] in doubles inside one 12 x 12 table
constexpr int qmpc_e_plain(int u, int v) { return u * QMPC_E_DIM + v; }
