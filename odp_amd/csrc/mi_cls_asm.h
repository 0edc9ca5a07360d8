// mi_cls_asm.h -- the rule-program assembler (mi_cls_asm.cpp): a mi_cls.h
// table in, the device words (mi_cls_prog.h) and the facts the launch side
// needs about them out.  Host-only C++17, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

// A/B and test switches of one compile (MI_CLS_NO_BV, MI_CLS_NO_JOINT,
// MI_CLS_NO_WIDE, MI_CLS_NO_CAND1, MI_CLS_NO_PORTMERGE, MI_CLS_NO_FLAT,
// MI_CLS_NO_PLAN, MI_CLS_VERBOSE; MI_CLS_DIV=0|1 forces the tree choice)
struct MiAsmKnobs {
	bool no_bv = false, no_joint = false, no_wide = false, no_cand1 = false, no_portmerge = false,
	     no_flat = false, no_plan = false, verbose = false;
	int div = -1;            // -1: by the program
};

MiAsmKnobs mi_asm_knobs_from_env();   // the unit's only reads of the environment

struct MiProgram {
	std::vector<uint32_t> w;     // device words
	uint32_t hot_words = 0;      // size of the hot region
	bool tree = false;           // some rule leads to a CoS with rules (DIV kernels)
	int flat_mode = -1;          // engine of the default CoS's block when one round on it
	                             // decides every packet (flat kernels), else -1
	int spec_mode = -1;          // engine a specialised kernel compiles in: flat_mode, or
	                             // FM_CHAIN for a flat program with a chain of blocks
	std::vector<uint32_t> plan;  // joint group per round of a CoS tree (tree-plan kernels)
};

// Validate the table (every index the kernels follow stays inside it), then
// assemble it.  0, -EINVAL (malformed table) or -E2BIG.
int mi_asm_compile(const void *tbl, size_t bytes, const MiAsmKnobs &kn, MiProgram &out);

// The hipRTC program of the specialised kernel of `p` (which has a
// spec_mode or a plan) for block shape nw / lt; ck: the pktin-option
// instantiation.  inst = the kernel instantiation's name expression.
std::string mi_asm_spec_program(const MiProgram &p, int nw, bool lt, bool ck, std::string &inst);
