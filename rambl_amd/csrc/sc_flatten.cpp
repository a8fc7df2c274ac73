// Level-major flattening of a PoGraph for the device.  See sc_graph.hpp.  The level walk reproduces
// the reference's StrainCall/NonparametricClustering.cpp:284-334 and :556-575.
#include "sc_graph.hpp"
#include "sc_phase_timer.hpp"

#include <algorithm>

namespace sc {

namespace {

// Symbol codes (A C G T - = first, every further symbol in the order code() first meets it) and the coded text of the read
// labels, each stored once in f.labels where offset() first meets it.  The order of the calls decides K, sym, code_N and
// every ent_lab_off.
struct LabelCoder {
    const PoGraph& g;
    FlatGraph& f;
    int code_of[256];
    std::vector<int> off, len;                                  // per labtab entry: where its codes start (-1: not yet coded)
    LabelCoder(const PoGraph& g, FlatGraph& f) : g(g), f(f), off(g.labtab.size(), -1), len(g.labtab.size(), 0) {
        static const char alpha[6] = {'A', 'C', 'G', 'T', '-', '='};
        f.sym.assign(alpha, alpha + 6);
        f.K = 6;
        for (int i = 0; i < 256; i++) code_of[i] = -1;
        for (int i = 0; i < 6; i++) code_of[(unsigned char)alpha[i]] = i;
        for (size_t i = 0; i < g.labtab.size(); i++) len[i] = (int)g.labtab[i].size();
    }
    uint8_t code(char c) {
        int& k = code_of[(unsigned char)c];
        if (k < 0) { k = f.K++; f.sym.push_back(c); if (c == 'N') f.code_N = k; }
        return (uint8_t)k;
    }
    int offset(int lab) {
        int lo = off[(size_t)lab];
        if (lo < 0) {
            lo = off[(size_t)lab] = (int)f.labels.size();
            for (char c : g.labtab[(size_t)lab]) f.labels.push_back(code(c));
        }
        return lo;
    }
};

// The node arrays, the out-edge CSR and the pool offsets, in final-id order; returns the number of pool entries.
size_t flatten_nodes(const PoGraph& g, const std::vector<int>& alive, LabelCoder& lc, FlatGraph& f) {
    f.n_nodes = (int)alive.size();
    f.node_lab_off.resize(f.n_nodes); f.node_lab_len.resize(f.n_nodes);
    f.node_label_str.resize(f.n_nodes); f.node_is_end.assign(f.n_nodes, 0);
    f.out_ptr.assign(f.n_nodes + 1, 0);
    f.pool_ptr.assign(f.n_nodes + 1, 0);
    size_t n_pool = 0, n_lab = 0, n_out = 0;
    for (int a = 0; a < f.n_nodes; a++) {
        const GNode& x = g.nodes[alive[a]];
        n_pool += x.pool.size(); n_out += x.out.size(); n_lab += x.lab.size();
    }
    f.pool_rid.resize(n_pool); f.pool_cn.resize(n_pool); f.out_node.reserve(n_out); f.labels.reserve(n_lab);
    for (int a = 0; a < f.n_nodes; a++) {
        const GNode& x = g.nodes[alive[a]];
        f.node_label_str[a] = x.lab;
        f.node_lab_off[a] = (int)f.labels.size();
        f.node_lab_len[a] = (int)x.lab.size();
        bool special = (x.lab == "^" || x.lab == "$");
        f.node_is_end[a] = (x.lab == "$");
        for (char c : x.lab) f.labels.push_back(special ? (uint8_t)0xFF : lc.code(c));
        f.out_ptr[a + 1] = f.out_ptr[a] + (int)x.out.size();
        for (int o : x.out) f.out_node.push_back(g.nodes[o].id);
        f.pool_ptr[a + 1] = f.pool_ptr[a] + (int)x.pool.size();
    }
    f.out_support.assign(f.out_node.size(), 0);
    return n_pool;
}

// The pools in node order for the edge-support kernel.
void copy_pools(const PoGraph& g, const std::vector<int>& alive, int threads, FlatGraph& f) {
    std::atomic<bool> sorted{true};
    parallel_items(f.n_nodes, threads, [&](int a) {
        const GNode& x = g.nodes[alive[a]];
        int prev = -1;
        int* pr = f.pool_rid.data() + f.pool_ptr[a]; int* pc = f.pool_cn.data() + f.pool_ptr[a];
        size_t k = 0;
        bool ok = true;
        for (const auto& e : x.pool) {
            pr[k] = e.rid; pc[k] = e.cn; k++;
            if (e.rid < prev) ok = false;
            prev = e.rid;
        }
        if (!ok) sorted.store(false, std::memory_order_relaxed);
    });
    if (!sorted.load()) f.pools_sorted = false;
}

const size_t NO_ENTRIES = SIZE_MAX;

// The order of the walk alone, breadth first over the nodes: the nodes of every level, whether and where "$" is among them,
// and in ent_at, per walked node, where its entries go (NO_ENTRIES for "^" and "$").  Sizes the ent_* arrays.
void walk_levels(const PoGraph& g, const std::vector<int>& alive, FlatGraph& f, std::vector<size_t>& ent_at) {
    std::vector<int> level_node{0}, sub;
    std::vector<int> visited(f.n_nodes, -1);
    size_t ne = 0;
    f.level_node_ptr.push_back(0);
    f.level_ent_ptr.push_back(0);
    for (int level = 0; !level_node.empty(); level++) {
        int end_pos = -1;
        for (size_t qi = 0; qi < level_node.size(); qi++) {
            const int a = level_node[qi];
            const GNode& x = g.nodes[alive[a]];
            f.level_nodes.push_back(a);
            if (a == 0) ent_at.push_back(NO_ENTRIES);
            else if (f.node_is_end[a]) { end_pos = (int)qi; ent_at.push_back(NO_ENTRIES); }
            else { ent_at.push_back(ne); ne += x.pool.size(); }
            for (int o : x.out) {
                const int b = g.nodes[o].id;
                if (visited[b] != level) { sub.push_back(b); visited[b] = level; }
            }
        }
        f.level_node_ptr.push_back((int)f.level_nodes.size());
        f.level_ent_ptr.push_back((int)ne);
        f.level_has_end.push_back(end_pos >= 0);
        f.level_end_pos.push_back(end_pos);
        level_node.swap(sub);
        sub.clear();
    }
    f.n_levels = (int)f.level_has_end.size();
    f.ent_rid.resize(ne); f.ent_cn.resize(ne); f.ent_lab_off.resize(ne); f.ent_lab_len.resize(ne); f.ent_first.resize(ne);
    f.level_read_count.assign((size_t)f.n_levels, 0);
}

// The entries of one level.  A read's first occurrence within the level is stamped in the caller's rid_stamp; label_off(lab)
// gives where the codes of a label start.  Returns the level's read count.
// (A single-character strain label against a multi-character read label is modelled on the device: the reference looks up
// the never-set key sub_count[(c, "multi")] -> log 0, k_level.)
template <class LabelOff>
int fill_level(const PoGraph& g, const std::vector<int>& alive, const std::vector<size_t>& ent_at, const std::vector<int>& lab_len,
               int level, std::vector<int>& rid_stamp, FlatGraph& f, const LabelOff& label_off) {
    int lrc = 0;
    for (int it = f.level_node_ptr[(size_t)level]; it < f.level_node_ptr[(size_t)level + 1]; it++) {
        const size_t at = ent_at[(size_t)it];
        if (at == NO_ENTRIES) continue;
        const GNode& x = g.nodes[alive[f.level_nodes[(size_t)it]]];
        int* er = f.ent_rid.data() + at; int* ec = f.ent_cn.data() + at;
        int* eo = f.ent_lab_off.data() + at; int* el = f.ent_lab_len.data() + at; uint8_t* ef = f.ent_first.data() + at;
        size_t k = 0;
        for (const auto& e : x.pool) {
            er[k] = e.rid; ec[k] = e.cn;
            eo[k] = label_off(e.lab); el[k] = lab_len[(size_t)e.lab];
            if ((size_t)e.rid >= rid_stamp.size()) rid_stamp.resize((size_t)e.rid + 1, -1);
            ef[k] = rid_stamp[(size_t)e.rid] != level;
            rid_stamp[(size_t)e.rid] = level;
            lrc += e.cn;
            k++;
        }
    }
    return lrc;
}

// Codes every label ahead of the fill, as filling the levels in order would: in parallel over the walk's nodes, the labels
// each pool carries in the order it first carries them; then, in walk order, the coding of those not yet coded.
void code_labels_in_walk_order(const PoGraph& g, const std::vector<int>& alive, const std::vector<size_t>& ent_at, int threads,
                               const FlatGraph& f, LabelCoder& lc) {
    const int n_items = (int)f.level_nodes.size();
    std::vector<std::vector<int>> firsts((size_t)n_items);
    parallel_items(n_items, threads, [&] { return std::vector<int>(g.labtab.size(), -1); }, [&](int it, std::vector<int>& seen) {
        if (ent_at[(size_t)it] == NO_ENTRIES) return;
        for (const auto& e : g.nodes[alive[f.level_nodes[(size_t)it]]].pool)
            if (seen[(size_t)e.lab] != it) { seen[(size_t)e.lab] = it; firsts[(size_t)it].push_back(e.lab); }
    });
    for (int it = 0; it < n_items; it++)
        for (int lab : firsts[(size_t)it]) lc.offset(lab);
}

}  // namespace

void flatten(const PoGraph& g, int n_reads, FlatGraph& f) {
    PhaseTimer tp("  flatten phase ", 16);
    LabelCoder lc(g, f);
    std::vector<int> alive;
    for (int i = 0; i < (int)g.nodes.size(); i++) if (g.nodes[i].alive) alive.push_back(i);
    const int threads = graph_threads((long)flatten_nodes(g, alive, lc, f));
    copy_pools(g, alive, threads, f);
    tp.phase("nodes + pools");

    // A million entries per region (88 M on a deep one), written by index; this was more than half of a region's set-up on
    // the host.  The first occurrence of a read is a matter of one level, so the levels fill independently of each other,
    // but symbol codes are handed out in the order the entries are walked.  On one thread a label is coded where an entry
    // first carries it; on several, all of them ahead of the fill.
    std::vector<size_t> ent_at;
    walk_levels(g, alive, f, ent_at);
    auto stamps = [&] { return std::vector<int>((size_t)std::max(n_reads, 1), -1); };
    if (threads > 1) {
        code_labels_in_walk_order(g, alive, ent_at, threads, f, lc);
        parallel_items(f.n_levels, threads, stamps, [&](int level, std::vector<int>& rid_stamp) {
            f.level_read_count[(size_t)level] =
                fill_level(g, alive, ent_at, lc.len, level, rid_stamp, f, [&](int lab) { return lc.off[(size_t)lab]; });
        });
    } else {
        std::vector<int> rid_stamp = stamps();
        for (int level = 0; level < f.n_levels; level++)
            f.level_read_count[(size_t)level] =
                fill_level(g, alive, ent_at, lc.len, level, rid_stamp, f, [&](int lab) { return lc.offset(lab); });
    }
    tp.phase("level walk");
    if (f.K > 16 && f.unsupported.empty()) f.unsupported = "more than 16 distinct symbols in node/read labels";
}

}  // namespace sc
