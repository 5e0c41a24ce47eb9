// cf_rank_cli.hpp -- what recommend, rankeval and ease share after the scores: the --users file, the
// held-out CSR, the list and rank files and the printed lines.  One writer and one printer per
// format, so the three binaries cannot drift apart.
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
#include "cf_mf_cli.hpp"

namespace cfrank {

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

// The lists of n_out users (sel[j] when selected, else j), N slots each.
inline void write_lists(const std::string& output, int nshards, const cfio::IdMap& uids, const cfio::IdMap& mids,
                        bool selected, const std::vector<uint32_t>& sel, uint32_t n_out, uint32_t N,
                        const std::vector<uint32_t>& items, const std::vector<double>& scores,
                        const std::vector<uint32_t>& count) {
    cfio::ShardWriter w(".", output, nshards);
    for (uint32_t j = 0; j < n_out; ++j) {
        const uint32_t uid = uids.ids[selected ? sel[j] : j];
        std::string& out = w.shard(uid);
        for (uint32_t r = 0; r < count[j]; ++r) {
            cfio::append_u(out, uid);
            out += '\t';
            cfio::append_u(out, mids.ids[items[(size_t)j * N + r]]);
            out += '\t';
            cfio::append_g(out, scores[(size_t)j * N + r]);
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
