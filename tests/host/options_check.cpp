// The switch table (eorb_slam_amd/csrc/eorb_options.h) from a plain C++ caller.  One scenario per input line:
//   NAME=value NAME=value ... | name value name value ...
// environment entries (handed to options_from_env through a fake lookup), then option calls in order.  Per scenario:
//   opt <row> <value>        every row after the calls
//   knob <field> <value>     accum_knobs(opt, 512)
//   call <name> <known>      every option call
//   end
// With the argument "table": one line `row <option> <environment or -> <default> <unset>` per row of kOptions.
// (tests/test_options_cpp.py)
#include <stdio.h>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>
#include "eorb_slam_amd/csrc/eorb_options.h"

using namespace eorb;

static std::map<std::string, std::string> g_env;
static const char* fake_env(const char* name)
{
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "table") {
        for (const OptionRow& r : kOptions) printf("row %s %s %lld %d\n", r.name, r.env ? r.env : "-", r.dflt, (int)r.unset);
        return 0;
    }
    char line[8192];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string tok;
        g_env.clear();
        while (in >> tok && tok != "|") {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad environment entry '%s'\n", tok.c_str()); return 1; }
            g_env[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        const Options created = options_from_env(fake_env);
        Options opt = created;
        std::vector<std::pair<std::string, bool>> calls;
        long long value;
        while (in >> tok >> value) calls.emplace_back(tok, option_set(opt, created, tok.c_str(), value));
        for (const OptionRow& r : kOptions) {
            long long v = 0;
            if (!option_get(opt, r.name, &v)) { fprintf(stderr, "row '%s' cannot be read\n", r.name); return 1; }
            printf("opt %s %lld\n", r.name, v);
        }
        const AccumKnobs k = accum_knobs(opt, 512);
        printf("knob gather_form %d\nknob dd_min %lld\nknob pd %d\nknob scatter %d\nknob gather_threads %d\nknob gather_nc %d\n", k.gather_form,
               (long long)k.dd_min, k.pd, k.scatter, k.gather_threads, k.gather_nc);
        printf("knob slot_chunk %d\nknob slot_waves %d\nknob slot_rounds %d\nknob slot_rank %d\nknob slot_hot_min %lld\n", k.slot_chunk, k.slot_waves,
               k.slot_rounds, (int)k.slot_rank, k.slot_hot_min);
        printf("knob slot_hot_cap %d\nknob slot_hot_waves %d\nknob slot_prerank %d\nknob slot_halves %d\n", k.slot_hot_cap, k.slot_hot_waves,
               k.slot_prerank, k.slot_halves);
        for (const auto& c : calls) printf("call %s %d\n", c.first.c_str(), (int)c.second);
        printf("end\n");
    }
    return 0;
}
