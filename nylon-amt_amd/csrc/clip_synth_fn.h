// The two transcendental functions of the clip synth (clip_synth.hip), defined once: the kernel and tools/synth_fn_error.hip, which measures
// them against fp64, call these and nothing else.  Both are single hardware instructions of gfx950.
#pragma once
#include "hftt_common.h"

// S(u) = sin(2 pi u), u in turns (v_sin_f32; the contract keeps u inside [-0.5, 0.5], far inside the instruction's domain of +-256 turns)
__device__ __forceinline__ float synth_sin_turns(float u) { return __builtin_amdgcn_sinf(u); }

// E(y) = 2^y (v_exp_f32); the caller keeps y inside [-126, 0], where the result is a normal number
__device__ __forceinline__ float synth_exp2(float y) { return __builtin_amdgcn_exp2f(y); }
