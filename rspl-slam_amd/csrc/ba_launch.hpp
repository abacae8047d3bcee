// Local BA, private to its three units: the host launch functions ba_schur.hip offers the trial entry
// points of ba_trial.hip (ba_first.hip needs none).  A kernel is defined, launched and given its
// attributes in one unit only; no kernel is declared across units.
#pragma once
#include "ba_kernels.hpp"

namespace rspl {
namespace ba {

// Schur chunks; with wave_fused (wave_path(A.K) only) the last pose pair also solves
void launch_chunks(const Problem& P, const Lin& L, const Active& A, const Sys& S, double lambda, const Lin& Ls,
                   const Sys& Ss, bool wave_fused, hipStream_t s);
// the reduced-system solve of a fast_path window (the K ranges: at its definition)
hipError_t launch_solve(const Problem& P, const Active& A, const Sys& S, double lambda, hipStream_t s,
                        bool wave_fused);
// windows beyond fast_path: pose-pair sums into S.S, Cholesky in global memory
void launch_global_solve(const Active& A, const Sys& S, double lambda, hipStream_t s);

}  // namespace ba
}  // namespace rspl
