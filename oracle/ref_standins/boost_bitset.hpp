// TEST INFRASTRUCTURE ONLY.  Stand-in for `typedef boost::dynamic_bitset<> boost_bitset_t` (the reference's
// lib/types.hpp, which the build skips because Boost is not installed here).  Block.cc uses the type only in
// getNoBlocksContigs / the ".noblocks" bookkeeping, which the merge-block driver never calls; the methods below are
// the ones those functions name, so that Block.cc compiles unchanged.  Force-included (-include) by oracle/Makefile.
#ifndef GAMREF_STANDIN_BOOST_BITSET
#define GAMREF_STANDIN_BOOST_BITSET
#include <cstddef>
#include <vector>

class boost_bitset_t {
    std::vector<bool> bits_;

public:
    boost_bitset_t() {}
    explicit boost_bitset_t(std::size_t n) : bits_(n) {}
    std::size_t size() const { return bits_.size(); }
    void reset() { bits_.assign(bits_.size(), false); }
    void set(std::size_t i) { bits_.at(i) = true; }
    bool test(std::size_t i) const { return bits_.at(i); }
    void flip() { bits_.flip(); }
    std::vector<bool>::reference operator[](std::size_t i) { return bits_[i]; }
    bool operator[](std::size_t i) const { return bits_[i]; }
    boost_bitset_t& operator|=(const boost_bitset_t& o)
    {
        for (std::size_t i = 0; i < bits_.size() && i < o.bits_.size(); i++)
            if (o.bits_[i]) bits_[i] = true;
        return *this;
    }
};
#endif
