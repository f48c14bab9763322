// launch_plan_main -- prints what urmap_amd/csrc/launch_plan.h decides (tests/test_launch_plan_cpu.py compiles it with g++ under
// ASan + UBSan and reads the output).
//   launch_plan_main              one line per combination of inputs: the inputs | the first pass's kernels | phase6=0/1
//   launch_plan_main bounds STR   what URMAPX_DP_BOUNDS=STR gives over the short reads' default: "rounds lo0 lo1 ..."
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../urmap_amd/csrc/launch_plan.h"

using namespace urx;

static std::string name(const SearchInstance &i) {
	char b[96];
	snprintf(b, sizeof b, "search_se_kernel<%d, %s, %s, %d, %d, %d>", i.nch, i.ovf ? "true" : "false", i.dbg ? "true" : "false", i.rows, i.part, i.kch);
	return b;
}

int main(int argc, char **argv) {
	if (argc == 3 && !strcmp(argv[1], "bounds")) {
		const DpBounds b = parse_dp_bounds(argv[2], dp_bounds_default(false));
		printf("%d", b.rounds);
		for (int i = 0; i <= DP_ROUNDS; ++i) printf(" %u", b.lo[i]);
		printf("\n");
		return 0;
	}
	const int classes[] = {2, 3, 4, 5, 8, 16};
	const uint32_t lens[] = {150, 151, 152, 192};
	for (int nch : classes)
		for (int bits = 0; bits < 64; ++bits)
			for (uint32_t len : lens) {
				SearchPlanIn in;
				in.nch = nch;
				in.rowinfo = bits & 1; in.slot16 = bits & 2; in.stats = bits & 4; in.dp0 = bits & 8; in.dp3 = bits & 16; in.no_k2 = bits & 32;
				in.dp_blocks = in.dp0 ? 1024 : 0;
				in.max_read_len = len; in.W = 24;
				const SearchPlan p = plan_search_se(in);
				SearchInstance i = first_pass_instance(p.first, nch);
				std::string kernels = name(i);
				if (p.first == FirstPass::ParkedPhase3) {
					i.part = 2;
					kernels += " + dp_kernel<" + std::to_string(nch) + "> + " + name(i);
				}
				printf("nch=%d rowinfo=%d slot16=%d stats=%d phase6=%d park3=%d len=%u no_k2=%d | %s | phase6=%d | second: %s\n", nch, in.rowinfo, in.slot16,
				       in.stats, in.dp0, in.dp3, len, in.no_k2, kernels.c_str(), p.phase6_launches, name(second_pass_instance(nch)).c_str());
			}
	return 0;
}
