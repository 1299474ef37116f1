// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// C-ABI shim around the reference's own merge-block (L1) driver, built by oracle/Makefile into
// oracle/_ref/libgaml1ref.so (git-ignored) so that oracle/gamdp_oracle.c's gamdp_oracle_align_merge_block and the
// device path can be pinned against it (tests/golden/make_golden_l1_vs_ref.py, tests/test_l1_oracle_vs_ref.py).
//
// The five functions themselves -- PctgBuilder::alignMergeBlock, findBestAlignment, alignBlocks and both is_good
// overloads (lib/src/pctg/PctgBuilder.cc:726-844, 1361-1731) -- are the reference's text, cut out of PctgBuilder.cc at
// build time by oracle/l1_extract.py into oracle/_ref/pctg_l1_bodies.inc and #included below.  What this file adds
// is only what those bodies name and the rest of PctgBuilder.cc would have supplied:
//
//   PctgBuilder            a class with the five methods (declared with the reference's parameter types) and
//                          loadMasterContig / loadSlaveContig, which hand back the two contigs of this call;
//   CompactAssemblyGraph   a class whose getBlocks(v) returns the block list of this call (the only use of the graph);
//   MergeBlock             the reference's own (pctg/MergeDescriptor.hpp);
//   Block / Frame / BestCtgAlignment / BandedSmithWaterman / ABlast / Contig
//                          the reference's own .cc files, compiled where they lie (oracle/Makefile).
//
// Every BandedSmithWaterman::find_alignment call the bodies make goes through gamref_l1_wrap_find_alignment
// (the linker's --wrap): it records the call -- which contig each side is (master, slave, or the slave's reverse
// complement, and the offset of a chopped tail in it), the four window bounds, the force flags and the result -- and
// then returns exactly what the reference's find_alignment returned (or rethrows what it threw).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <list>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "alignment/ablast.hpp"
#include "alignment/banded_smith_waterman.hpp"
#include "alignment/my_alignment.hpp"
#include "assembly/Block.hpp"
#include "assembly/Frame.hpp"
#include "assembly/contig.hpp"
#include "pctg/BestCtgAlignment.hpp"
#include "pctg/MergeDescriptor.hpp"

#define GAMREF_API extern "C" __attribute__((visibility("default")))

class CompactAssemblyGraph {
public:
    typedef uint64_t Vertex;
    explicit CompactAssemblyGraph(const std::list<Block>& blocks) : blocks_(blocks) {}
    const std::list<Block>& getBlocks(const Vertex&) const { return blocks_; }

private:
    const std::list<Block>& blocks_;
};

class PctgBuilder {
public:
    PctgBuilder(const Contig& master, const Contig& slave) : master_(master), slave_(slave) {}

    const Contig& loadMasterContig(const int32_t) const { return master_; }
    const Contig& loadSlaveContig(const int32_t) const { return slave_; }

    void alignMergeBlock(const CompactAssemblyGraph&, MergeBlock&) const;
    void findBestAlignment(BestCtgAlignment&, Contig&, uint64_t, uint64_t, Contig&, uint64_t, uint64_t,
                           const std::list<Block>&) const;
    void alignBlocks(const Contig&, const uint64_t&, const Contig&, const uint64_t&, const std::list<Block>&,
                     std::vector<MyAlignment>&) const;
    bool is_good(const std::vector<MyAlignment>&, uint64_t) const;
    bool is_good(const MyAlignment&, uint64_t) const;

private:
    const Contig& master_;
    const Contig& slave_;
};

#include "pctg_l1_bodies.inc"

extern "C" {

// same layout as gamdp_oracle_block / gamdp_oracle_mb (oracle/gamdp_oracle.h), so that both take the same inputs
struct gamref_l1_block {
    int32_t m_begin, m_end, s_begin, s_end;
    char m_strand, s_strand;
    int64_t n_reads;
};

struct gamref_l1_mb {
    uint8_t m_ltail, m_rtail, s_ltail, s_rtail;  // in
    uint8_t align_ok, align_rev, status, touched;  // out; status 0 ok, 2 std::out_of_range, 3 other exception
    int32_t m_start, m_end, s_start, s_end;        // out (meaningful only if touched)
    uint32_t n_dp;                                  // find_alignment calls made
    uint64_t cells;                                 // not known to the reference: left 0
};

// one find_alignment call of the reference
struct gamref_l1_call {
    char a_tag, b_tag;  // 'M' master, 'S' slave as given, 'R' its reverse complement, '?' none of them
    uint8_t force_start, force_end, status;  // status 0 returned, 2 threw std::out_of_range, 3 threw something else
    uint8_t first_found, last_found, pad_;
    uint64_t a_off, b_off;  // the contig is the tag's sequence from this offset on (a tail cut by chop_begin)
    uint64_t begin_a, end_a, begin_b, end_b;  // the window as passed
    // the returned MyAlignment and first_match_pos / last_match_pos of it
    uint64_t r_begin_a, r_begin_b, r_a_size, r_b_size, length, n_match;
    int64_t score;
    double homology;
    uint64_t first_a, first_b, last_a, last_b;
};

}  // extern "C"

namespace {

struct Trail {
    std::string master, slave, slave_rc;
    gamref_l1_call* calls;
    uint32_t cap, n;
};
thread_local Trail* g_trail = nullptr;

Contig make_contig(const char* s, uint64_t n)
{
    Contig c(std::string("c"), size_t(n));
    for (uint64_t i = 0; i < n; i++) c.at(i) = s[i];  // Nucleotide::operator=(char)
    return c;
}

std::string chars(const Contig& c)
{
    std::string s(c.size(), 'N');
    for (size_t i = 0; i < c.size(); i++) s[i] = char(c.at(i));
    return s;
}

void identify(const Trail& t, const Contig& c, char* tag, uint64_t* off)
{
    const std::string s = chars(c);
    const std::pair<char, const std::string*> views[3] = {{'M', &t.master}, {'S', &t.slave}, {'R', &t.slave_rc}};
    for (const auto& v : views)
        if (s.size() <= v.second->size() && v.second->compare(v.second->size() - s.size(), s.size(), s) == 0) {
            *tag = v.first;
            *off = v.second->size() - s.size();
            return;
        }
    *tag = '?';
    *off = 0;
}

}  // namespace

typedef BandedSmithWaterman::size_type bsw_size;
MyAlignment gamref_l1_real_find_alignment(const BandedSmithWaterman* self, const Contig& a, bsw_size begin_a,
                                          bsw_size end_a, const Contig& b, bsw_size begin_b, bsw_size end_b,
                                          bool force_start, bool force_end)
    __asm__("__real__ZNK19BandedSmithWaterman14find_alignmentERK6ContigmmS2_mmbb");
MyAlignment gamref_l1_wrap_find_alignment(const BandedSmithWaterman* self, const Contig& a, bsw_size begin_a,
                                          bsw_size end_a, const Contig& b, bsw_size begin_b, bsw_size end_b,
                                          bool force_start, bool force_end)
    __asm__("__wrap__ZNK19BandedSmithWaterman14find_alignmentERK6ContigmmS2_mmbb") __attribute__((used));

MyAlignment gamref_l1_wrap_find_alignment(const BandedSmithWaterman* self, const Contig& a, bsw_size begin_a,
                                          bsw_size end_a, const Contig& b, bsw_size begin_b, bsw_size end_b,
                                          bool force_start, bool force_end)
{
    Trail* t = g_trail;
    gamref_l1_call rec;
    std::memset(&rec, 0, sizeof(rec));
    if (t) {
        identify(*t, a, &rec.a_tag, &rec.a_off);
        identify(*t, b, &rec.b_tag, &rec.b_off);
    }
    rec.begin_a = begin_a;
    rec.end_a = end_a;
    rec.begin_b = begin_b;
    rec.end_b = end_b;
    rec.force_start = force_start;
    rec.force_end = force_end;
    struct Record {  // appends rec to the trail however the call ends
        Trail* t;
        gamref_l1_call& rec;
        ~Record()
        {
            if (!t) return;
            if (t->n < t->cap) t->calls[t->n] = rec;
            t->n++;
        }
    } record{t, rec};
    try {
        MyAlignment r = gamref_l1_real_find_alignment(self, a, begin_a, end_a, b, begin_b, end_b, force_start, force_end);
        rec.r_begin_a = r.begin_a();
        rec.r_begin_b = r.begin_b();
        rec.r_a_size = r.a_size();
        rec.r_b_size = r.b_size();
        rec.score = r.score();
        rec.homology = r.homology();
        rec.length = r.length();
        uint64_t nm = 0;
        for (uint64_t i = 0; i < r.sequence().size(); i++) nm += r.sequence()[i] == MATCH;
        rec.n_match = nm;
        std::pair<uint64_t, uint64_t> p;
        rec.first_found = first_match_pos(r, p) ? 1 : 0;
        rec.first_a = p.first;
        rec.first_b = p.second;
        rec.last_found = last_match_pos(r, p) ? 1 : 0;
        rec.last_a = p.first;
        rec.last_b = p.second;
        return r;
    } catch (const std::out_of_range&) {
        rec.status = 2;
        throw;
    } catch (...) {
        rec.status = 3;
        throw;
    }
}

// PctgBuilder::alignMergeBlock on one merge block: master / slave are ACGTN chars, blocks in the graph's list order.
// out->m_ltail..s_rtail are read; the rest is written.  trail (optional) receives up to trail_cap calls.
// Returns out->status.
GAMREF_API int gamref_align_merge_block(const char* master, uint64_t mlen, const char* slave, uint64_t slen,
                                        const gamref_l1_block* blocks, uint32_t nb, gamref_l1_mb* out,
                                        gamref_l1_call* trail, uint32_t trail_cap)
{
    Trail t;
    t.master.assign(master, mlen);
    t.slave.assign(slave, slen);
    t.calls = trail;
    t.cap = trail ? trail_cap : 0;
    t.n = 0;
    const uint8_t tails[4] = {out->m_ltail, out->m_rtail, out->s_ltail, out->s_rtail};
    std::memset(out, 0, sizeof(*out));
    std::memcpy(&out->m_ltail, tails, 4);
    try {
        Contig m = make_contig(master, mlen), s = make_contig(slave, slen);
        t.master = chars(m);  // normalised the way the reference's Contig holds them
        t.slave = chars(s);
        Contig rc(s);
        reverse_complement(rc);
        t.slave_rc = chars(rc);
        std::list<Block> blist;
        for (uint32_t k = 0; k < nb; k++) {
            Block b;
            b.setMasterFrame(Frame(0, blocks[k].m_strand, blocks[k].m_begin, blocks[k].m_end));
            b.setSlaveFrame(Frame(0, blocks[k].s_strand, blocks[k].s_begin, blocks[k].s_end));
            b.setReadsNumber(blocks[k].n_reads);
            blist.push_back(b);
        }
        CompactAssemblyGraph graph(blist);
        PctgBuilder pb(m, s);
        MergeBlock mb;
        std::memset(&mb, 0, sizeof(mb));
        mb.vertex = 0;
        mb.m_ltail = tails[0];
        mb.m_rtail = tails[1];
        mb.s_ltail = tails[2];
        mb.s_rtail = tails[3];
        const int32_t unset = INT32_MIN;  // alignMergeBlock writes all four coordinates or none
        mb.m_start = mb.m_end = mb.s_start = mb.s_end = unset;
        g_trail = &t;
        pb.alignMergeBlock(graph, mb);
        g_trail = nullptr;
        out->align_ok = mb.align_ok;
        out->align_rev = mb.align_rev;
        out->touched = mb.m_start != unset || mb.m_end != unset || mb.s_start != unset || mb.s_end != unset;
        if (out->touched) {
            out->m_start = mb.m_start;
            out->m_end = mb.m_end;
            out->s_start = mb.s_start;
            out->s_end = mb.s_end;
        }
        out->status = 0;
    } catch (const std::out_of_range&) {
        out->status = 2;
    } catch (...) {
        out->status = 3;
    }
    g_trail = nullptr;
    out->n_dp = t.n;
    return out->status;
}

// what the bodies were cut from: "PctgBuilder.cc:<sha256> PctgBuilder.hpp:<sha256>"
GAMREF_API const char* gamref_l1_sources_sha256() { return GAMREF_L1_SOURCES_SHA256; }
