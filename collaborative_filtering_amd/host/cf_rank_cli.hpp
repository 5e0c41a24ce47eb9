// cf_rank_cli.hpp -- what recommend, rankeval and ease share around the scores: the score source of
// --factors / --graph with its id maps, the exclusion CSR from the role edges, the --users selection
// with the list buffers, the held-out CSR, the list and rank files and the printed lines.  One loader,
// one writer and one printer per format, so the three binaries cannot drift apart.
//   R_<i>_of_<nshards>   lists: "user\titem\tscore" per listed item in rank order per user, score as %g
//                        ranks: "user\titem\trank\tn_cand" per held-out edge, by user then item; ranks
//                        are 0-based, a skipped edge (excluded, or a NaN score) has rank -1
//                        both sharded by user id like the predictions (cf_mf_cli.hpp write_predictions)
#pragma once

#include <algorithm>
#include <charconv>
#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#include "cf_cli.hpp"
#include "cf_factor_io.hpp"
#include "cf_knn_cli.hpp"
#include "cf_mf_cli.hpp"

namespace cfrank {

// The score source of recommend and rankeval: the factor files of --factors (with `bias` the bias
// files too), or the item graph of --graph with the profiles of DIR, uploaded into a context opened
// here (ctx stays null for factors: the caller opens it when it scores).
struct Source {
    cf_ctx* ctx = nullptr;
    bool from_graph = false;
    cfmf::Factors fu, fv;
    std::vector<double> bu, bi;
    cfknn::Source g;
    const cfio::IdMap& uids() const { return from_graph ? g.users : fu.ids; }
    const cfio::IdMap& mids() const { return from_graph ? g.items : fv.ids; }
    void print_sizes() const {
        if (from_graph) std::printf("Users: %u items: %u\n", uids().size(), mids().size());
        else std::printf("Users: %u items: %u D: %u\n", uids().size(), mids().size(), fu.width);
    }
};

inline void load_source(Source& s, const cfknn::Options& knn, const std::string& factors, const std::string& matrix,
                        bool bias) {
    s.from_graph = !knn.graph.empty();
    if (s.from_graph) {
        s.ctx = cfcli::open_device();
        s.g = cfknn::load(s.ctx, knn.graph, matrix);
        return;
    }
    s.fu = cfmf::read_factors(factors + ".U");
    s.fv = cfmf::read_factors(factors + ".V");
    if (s.fu.width != s.fv.width)
        cfcli::die("factor line of another width: " + factors + ".U holds " + std::to_string(s.fu.width) +
                   " values per line, " + factors + ".V " + std::to_string(s.fv.width));
    if (s.fu.width > CF_ALS_MAX_D)
        cfcli::die("D = " + std::to_string(s.fu.width) + " is above " + std::to_string(CF_ALS_MAX_D));
    if (bias) {
        s.bu = cfmf::read_bias(factors + ".bias.U", s.fu);
        s.bi = cfmf::read_bias(factors + ".bias.V", s.fv);
    }
}

// The edges of DIR whose role is in `excluded` (bit 1 << role) as a CSR by user in the source's
// indices, and with `held` the VALIDATE edges (user, item, value).  A user or item of DIR that the
// source does not hold is fatal, whatever the role of its edge.
inline cfmf::Csr role_exclusions(const Source& s, const std::string& matrix, const std::string& factors, unsigned excluded,
                                 std::vector<std::tuple<uint32_t, uint32_t, float>>* held) {
    const cfio::IdMap &uids = s.uids(), &mids = s.mids();
    std::vector<uint32_t> eu, em;
    for (const cfio::RoleRating& r : s.from_graph ? s.g.roles : cfio::load_movielens_roles(matrix)) {
        const auto u = uids.at.find(r.user);
        if (u == uids.at.end())
            cfcli::die("user " + std::to_string(r.user) + " of " + matrix + " has no line in " + factors + ".U_*");
        const auto m = mids.at.find(r.item);
        if (m == mids.at.end())
            cfcli::die("item " + std::to_string(r.item) + " of " + matrix + " has no line in " + factors + ".V_*");
        if (excluded >> r.role & 1u) {
            eu.push_back(u->second);
            em.push_back(m->second);
        }
        if (held && r.role == cfio::kValidate) held->emplace_back(u->second, m->second, r.obs);
    }
    cfmf::Csr excl = cfmf::build_csr(uids.size(), eu, em, std::vector<float>(eu.size(), 0.0f));
    if (excl.nbr.empty()) excl.nbr.push_back(0);   // a valid pointer for an empty list
    return excl;
}

// --users FILE: one user id per line, as compact indices in the file's order; an id that `uids`
// does not hold is fatal (`where` names the place a user id comes from).
inline std::vector<uint32_t> read_users(const std::string& users_file, const cfio::IdMap& uids, const std::string& where) {
    std::vector<uint32_t> sel;
    const std::string text = cfio::read_file(users_file);
    const char* p = text.data();
    const char* e = p + text.size();
    while (p < e) {
        if (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') {
            ++p;
            continue;
        }
        uint32_t id = 0;
        const auto r = std::from_chars(p, e, id);
        if (r.ec != std::errc()) cfcli::die("--users: " + users_file + " holds something that is not a user id");
        p = r.ptr;
        const auto u = uids.at.find(id);
        if (u == uids.at.end()) cfcli::die("user " + std::to_string(id) + " of " + users_file + " has no line in " + where);
        sel.push_back(u->second);
    }
    return sel;
}

inline void print_topn_stats(const cf_topn_stats& st) {
    std::printf("User blocks: %u  scoring kernels: %.3f ms  exclusion and selection kernels: %.3f ms\n", st.blocks,
                st.score_ms, st.select_ms);
    if (st.n_nan) std::printf("warning: %llu scores were NaN and are not listed\n", (unsigned long long)st.n_nan);
}

// The users whose lists are wanted (--users FILE, else all nu) and the buffers of their lists, N
// slots each; n_sel() / sel_ptr() are the selection arguments of cf_*_topn.
struct Lists {
    bool selected = false;
    std::vector<uint32_t> sel;   // never empty when selected: a valid pointer for an empty file
    uint32_t n_out = 0, N = 0;
    std::vector<uint32_t> items, count;
    std::vector<double> scores;
    uint32_t n_sel() const { return selected ? n_out : 0; }
    const uint32_t* sel_ptr() const { return selected ? sel.data() : nullptr; }
};

inline Lists make_lists(const std::string& users_file, const cfio::IdMap& uids, const std::string& where, uint32_t nu,
                        uint32_t N) {
    Lists l;
    l.selected = !users_file.empty();
    if (l.selected) l.sel = read_users(users_file, uids, where);
    l.n_out = l.selected ? (uint32_t)l.sel.size() : nu;
    if (l.selected && l.sel.empty()) l.sel.push_back(0);
    l.N = N;
    l.items.resize((size_t)l.n_out * N);
    l.count.resize(l.n_out);
    l.scores.resize((size_t)l.n_out * N);
    return l;
}

inline void write_lists(const std::string& output, int nshards, const cfio::IdMap& uids, const cfio::IdMap& mids,
                        const Lists& l) {
    cfio::ShardWriter w(".", output, nshards);
    for (uint32_t j = 0; j < l.n_out; ++j) {
        const uint32_t uid = uids.ids[l.selected ? l.sel[j] : j];
        std::string& out = w.shard(uid);
        for (uint32_t r = 0; r < l.count[j]; ++r) {
            cfio::append_u(out, uid);
            out += '\t';
            cfio::append_u(out, mids.ids[l.items[(size_t)j * l.N + r]]);
            out += '\t';
            cfio::append_g(out, l.scores[(size_t)j * l.N + r]);
            out += '\n';
        }
    }
    w.flush();
}

// The held-out edges as the CSR cf_*_rank_eval wants: by user, then item; the value of an edge is
// its weight.  A pair listed twice is fatal.
struct Held {
    std::vector<uint64_t> off;
    std::vector<uint32_t> item;   // never empty: valid pointers for an empty list
    std::vector<double> w;
    uint64_t n = 0;
};

inline Held build_held(std::vector<std::tuple<uint32_t, uint32_t, float>> held, uint32_t nu, const cfio::IdMap& uids,
                       const cfio::IdMap& mids, const std::string& matrix) {
    std::stable_sort(held.begin(), held.end(), [](const auto& a, const auto& b) {
        return std::get<0>(a) != std::get<0>(b) ? std::get<0>(a) < std::get<0>(b) : std::get<1>(a) < std::get<1>(b);
    });
    Held h;
    h.off.assign((size_t)nu + 1, 0);
    for (size_t e = 0; e < held.size(); ++e) {
        const uint32_t u = std::get<0>(held[e]), m = std::get<1>(held[e]);
        if (e && u == std::get<0>(held[e - 1]) && m == std::get<1>(held[e - 1]))
            cfcli::die("user " + std::to_string(uids.ids[u]) + " item " + std::to_string(mids.ids[m]) + " of " + matrix +
                       " is a VALIDATE edge twice");
        h.off[u + 1]++;
        h.item.push_back(m);
        h.w.push_back((double)std::get<2>(held[e]));
    }
    for (uint32_t u = 0; u < nu; ++u) h.off[u + 1] += h.off[u];
    h.n = h.item.size();
    if (h.item.empty()) {
        h.item.push_back(0);
        h.w.push_back(0.0);
    }
    return h;
}

inline void print_rank_summary(const cf_rank_summary& s, uint64_t n_held) {
    std::printf("Evaluated users: %u held-out edges: %llu skipped: %llu\n", s.users_evaluated, (unsigned long long)n_held,
                (unsigned long long)s.edges_skipped);
    std::printf("precision@N %g recall@N %g ndcg@N %g map@N %g mrr %g auc %g mpr %g\n", s.precision, s.recall, s.ndcg,
                s.map, s.mrr, s.auc, s.mpr);
    if (s.n_nan_held) std::printf("warning: %llu held-out scores were NaN and have no rank\n", (unsigned long long)s.n_nan_held);
}

inline void write_ranks(const std::string& output, int nshards, const cfio::IdMap& uids, const cfio::IdMap& mids,
                        const Held& h, const std::vector<uint32_t>& rank, const std::vector<cf_rank_user>& users) {
    const uint32_t nu = (uint32_t)(h.off.size() - 1);
    cfio::ShardWriter w(".", output, nshards);
    for (uint32_t u = 0; u < nu; ++u) {
        const uint32_t uid = uids.ids[u];
        for (uint64_t e = h.off[u]; e < h.off[u + 1]; ++e) {
            std::string& out = w.shard(uid);
            cfio::append_u(out, uid);
            out += '\t';
            cfio::append_u(out, mids.ids[h.item[e]]);
            out += '\t';
            if (rank[e] == 0xffffffffu) out += "-1";
            else cfio::append_u(out, rank[e]);
            out += '\t';
            cfio::append_u(out, users[u].n_cand);
            out += '\n';
        }
    }
    w.flush();
}

}  // namespace cfrank
