// TEST INFRASTRUCTURE ONLY.  Stand-in for Boost's <boost/detail/container_fwd.hpp> (Boost is not installed here).  The
// header only forward-declares standard containers; the files that include it also include the real standard headers,
// so an empty file is enough.
