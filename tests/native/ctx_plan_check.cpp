// The shape of a context without a GPU: prints sc::plan_context (rambl_amd/csrc/sc_plan.hpp) as one JSON line per
// argument tuple "stream_count:cu_count:cpus:local_world[:NAME=value[:NAME=value...]]", the options given explicitly
// (never read from the environment), next to sc::host_plan for the same tuple.  With no arguments: checks the
// Mersenne-twister restatement uniform_stream against <random>.
//   g++ -std=c++17 -o ctx_plan_check ctx_plan_check.cpp
#include <random>
#include <sstream>

#include "../../rambl_amd/csrc/sc_plan.hpp"

int main(int argc, char** argv) {
    if (argc == 1) {
        for (const int n : {4, 1000, 42048}) {
            const std::vector<double> u = sc::uniform_stream(1234u, n);
            std::mt19937 gen(1234);
            for (int i = 0; i < n; i++)
                if (u[(size_t)i] != std::generate_canonical<double, 53>(gen)) { printf("{\"uniform_ok\": false, \"at\": %d}\n", i); return 1; }
        }
        printf("{\"uniform_ok\": true}\n");
        return 0;
    }
    for (int a = 1; a < argc; a++) {
        std::vector<std::string> part;
        std::stringstream ss(argv[a]);
        for (std::string p; std::getline(ss, p, ':');) part.push_back(p);
        if (part.size() < 4) { fprintf(stderr, "bad tuple %s\n", argv[a]); return 2; }
        sc::Options o;
        for (size_t k = 4; k < part.size(); k++) {
            const size_t eq = part[k].find('=');
            if (eq == std::string::npos || !sc::set_option(o, part[k].substr(0, eq), part[k].c_str() + eq + 1)) { fprintf(stderr, "bad option %s\n", part[k].c_str()); return 2; }
        }
        const int streams = atoi(part[0].c_str()), cus = atoi(part[1].c_str()), world = atoi(part[3].c_str());
        const double cpus = atof(part[2].c_str());
        const sc::CtxPlan p = sc::plan_context(o, streams, cus, cpus, world);
        int hp[3] = {0, 0, 0};
        sc::host_plan(p.workers, world, cpus, hp);
        printf("{\"resident\": %d, \"res_slots\": %d, \"workers\": %d, \"launch_streams\": %d, \"setup_streams\": %d, \"exec_threads\": %d, "
               "\"long_threads\": %d, \"watch\": %d, \"server\": %d, \"arena_limit\": %d, \"setup_limit\": %d, \"host_plan\": [%d, %d, %d]}\n",
               (int)p.resident, p.res_slots, p.workers, p.launch_streams, p.setup_streams, p.exec_threads, p.long_threads, (int)p.watch,
               (int)p.server, p.arena_limit, p.setup_limit, hp[0], hp[1], hp[2]);
    }
    return 0;
}
