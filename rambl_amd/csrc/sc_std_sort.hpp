// libstdc++ std::sort permutation (the reference depends on its tie order at
// PartialOrderGraph.cpp:466, NonparametricClustering.cpp:647,675, StrainCall.cpp:1027).
#pragma once
#include <functional>
#include <vector>

namespace sc {

// less(a,b) compares element identities a,b (values stored in idx).
void std_sort_perm(std::vector<int>& idx, const std::function<bool(int, int)>& less);

}  // namespace sc
