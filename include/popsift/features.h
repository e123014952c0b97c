/*
 * popsift/features.h -- result containers of the drop-in API.
 * Replaces features.h:22-96 (Feature, FeaturesBase, FeaturesHost, typedef Features).
 * Layouts are the reference's: Feature keeps its four Descriptor* which point
 * into the FeaturesHost's own descriptor array.  FeaturesDev (features.h:98-118)
 * holds the results of an image in GPU memory and matches two such sets.
 */
#pragma once

#include <cmath>
#include <iostream>
#include <vector>

#include "sift_constants.h"
#include "sift_extremum.h"

struct popsift_hip_devfeatures;
struct popsift_hip_bytefeatures;
struct popsift_hip_gallery;

namespace popsift {

class FeaturesDevBytes;

struct Feature {
    int         debug_octave;
    float       xpos;
    float       ypos;
    float       sigma;
    int         num_ori;
    float       orientation[ORIENTATION_MAX_COUNT];
    Descriptor* desc[ORIENTATION_MAX_COUNT];

    void print(std::ostream& ostr, bool write_as_uchar) const;
};

std::ostream& operator<<(std::ostream& ostr, const Feature& feature);

class FeaturesBase {
    int _num_ext;
    int _num_ori;

public:
    FeaturesBase() : _num_ext(0), _num_ori(0) {}
    virtual ~FeaturesBase() {}

    inline int size() const { return _num_ext; }
    inline int getFeatureCount() const { return _num_ext; }
    inline int getDescriptorCount() const { return _num_ori; }

    inline void setFeatureCount(int num_ext) { _num_ext = num_ext; }
    inline void setDescriptorCount(int num_ori) { _num_ori = num_ori; }
};

class FeaturesHost : public FeaturesBase {
    Feature*         _ext;
    Descriptor*      _ori;
    unsigned char*   _bytes = 0;   /* byte format: num_ori x 128 bytes, a pinned block like the others */
    std::vector<int> _desc_idx;    /* byte format: ORIENTATION_MAX_COUNT descriptor indices per feature, -1 = none */
    std::vector<float> _responses; /* Config::setKeepStrongest only: one DoG response per feature */

public:
    FeaturesHost();
    FeaturesHost(int num_ext, int num_ori);
    virtual ~FeaturesHost();

    typedef Feature*       F_iterator;
    typedef const Feature* F_const_iterator;

    inline F_iterator       begin() { return _ext; }
    inline F_const_iterator begin() const { return _ext; }
    inline F_iterator       end() { return &_ext[size()]; }
    inline F_const_iterator end() const { return &_ext[size()]; }

    /* (re)allocates page-aligned arrays for num_ext features / num_ori descriptors */
    void reset(int num_ext, int num_ori);
    /* host-memory registration with the GPU runtime; no-ops here (the arrays already are
     * pinned blocks from a process-wide pool) but kept for source compatibility */
    void pin() {}
    void unpin() {}

    inline Feature*    getFeatures() { return _ext; }
    inline Descriptor* getDescriptors() { return _ori; } /* null in the byte format */

    /* Extension, Config::ByteDescriptors: (re)allocates num_ext features and num_ori descriptors of 128 bytes each (no
     * float descriptors: getDescriptors() and every Feature::desc[k] are null) */
    void resetBytes(int num_ext, int num_ori);
    bool hasDescriptorBytes() const { return _bytes != 0; }
    /* num_ori x 128 bytes (null in the float format); the D2H copy lands here */
    inline unsigned char* getDescriptorBytes() { return _bytes; }
    /* the 128 bytes of orientation `ori` of feature `feature`; null when ori >= num_ori (or in the float format) */
    const unsigned char* descriptorBytes(int feature, int ori) const;
    /* ORIENTATION_MAX_COUNT descriptor indices per feature (byte format; filled by PopSift's workers) */
    inline int* getDescriptorIndices() { return _desc_idx.data(); }

    /* Extension, Config::setKeepStrongest(n > 0): the DoG response of every feature (the strength the selection ranks by,
     * include/popsift_hip.h), in feature order; null when the setting is off (and for an image without features) */
    inline const float* getResponses() const { return _responses.empty() ? 0 : _responses.data(); }
    /* room for one response per feature (filled by PopSift's workers) */
    inline float* resetResponses() { _responses.assign((size_t)size(), 0.0f); return _responses.data(); }

    /* one line per (feature, orientation): x y 1/s^2 0 1/s^2 d0 .. d127; the byte format writes the bytes as
     * integers (the layout of write_as_uchar) */
    void print(std::ostream& ostr, bool write_as_uchar) const;
};

typedef FeaturesHost Features;

/* Extensions: the result arrays of FeaturesHost are pinned blocks from a process-wide pool; free blocks are cached for
 * reuse (POPSIFT_PINNED_CACHE_MB, default 2048) and released when the last PopSift object of the process is shut down.
 * releasePinnedCache() releases them at once; pinnedCacheBytes() tells how much is cached. */
void   releasePinnedCache();
size_t pinnedCacheBytes();
/* the NUMA node (or -1) whose free list serves the calling thread's result blocks; PopSift's workers set it */
void   setPinnedPoolNode(int node);
/* A block of the same pool (SiftJob keeps its copy of the caller's image in one: no allocation, no page faults and no
 * second staging copy per job).  *pinned tells whether the block is page-locked (it is not when no GPU runtime is there). */
void*  pinnedBlockGet(size_t bytes, bool* pinned);
void   pinnedBlockPut(void* block);

std::ostream& operator<<(std::ostream& ostr, const FeaturesHost& feature);

/*
 * Device-resident results of one image (PopSift in Config::MatchingMode, SiftJob::getDev()).
 * The three arrays live in the memory of the GPU that extracted the image: Feature records whose
 * desc[] point into the descriptor array, the descriptors, and the descriptor -> feature map.
 */
class FeaturesDev : public FeaturesBase {
    popsift_hip_devfeatures* _set;

public:
    FeaturesDev();
    FeaturesDev(int num_ext, int num_ori);
    /* takes ownership of a set made by the C ABI (popsift_hip_clone_results) */
    explicit FeaturesDev(popsift_hip_devfeatures* adopt);
    virtual ~FeaturesDev();

    void reset(int num_ext, int num_ori);

    /* brute-force 2-nearest-neighbour search of every descriptor of this set among the descriptors of
     * `other`; prints one "accept ..." / "reject ..." line per descriptor on stdout, as the reference does */
    void match(FeaturesDev* other);

    /* extension: the same search, results returned instead of printed */
    struct Match {
        int   best, second; /* descriptor indices in `other` */
        bool  accept;       /* dist_best / dist_second < 0.8 */
        float dist_best, dist_second; /* squared L2 */
    };
    std::vector<Match> matchAndGet(FeaturesDev* other);

    /* extension: correspondences instead of one row per descriptor (popsift_hip_match_pairs).  Descriptor i of this set
     * yields the pair (i, its nearest in `other`) iff dist_best / dist_second < ratio (0: no ratio test), dist_best <=
     * maxDist2, and -- with crossCheck -- i is the nearest descriptor of this set to that one (ties to the lower index).
     * Filtered on the GPU; pairs in ascending l.  The defaults give the rows matchAndGet accepts. */
    struct MatchOptions {
        float ratio = 0.8f;
        float maxDist2 = INFINITY; /* squared L2 */
        bool  crossCheck = false;
    };
    struct Pair {
        int   l, r;                 /* descriptor indices in this set and in `other` */
        float distBest, distSecond; /* squared L2 */
    };
    std::vector<Pair> matchPairs(FeaturesDev* other, const MatchOptions& opts);
    std::vector<Pair> matchPairs(FeaturesDev* other) { return matchPairs(other, MatchOptions()); }

    /* extension: guided matching (popsift_hip_match_pairs_guided; the rule is stated in popsift_hip.h).  With the model of
     * the image pair known -- popsift::Verifier's H or F, or any other -- descriptor i of this set is searched for only
     * among the descriptors of `other` whose feature lies within maxErr pixels of where the model puts i's: of its image
     * under the homography M (an affine map is one whose last row is 0 0 1), or of its epipolar line under the fundamental
     * matrix M (Sampson distance).  ratio, maxDist2 and crossCheck then act on those rows as in matchPairs; the
     * cross-check's search the other way round is guided too.  Both sets need features behind their descriptors. */
    struct GuidedOptions {
        enum Model { Homography = 0, Epipolar = 1 };
        Model model = Homography;
        float M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; /* row major: right ~ M * left, or [x' y' 1] M [x y 1]^T = 0 */
        float maxErr = 2.0f;                      /* pixels */
        float ratio = 0.8f;
        float maxDist2 = INFINITY;
        bool  crossCheck = false;
    };
    std::vector<Pair> matchGuided(FeaturesDev* other, const GuidedOptions& opts);
    /* the rows behind it, one per descriptor (popsift_hip_match_guided): best / second are -1 where there is none */
    std::vector<Match> matchGuidedRows(FeaturesDev* other, const GuidedOptions& opts);

    /* extension: a set of num descriptors (num x 128 floats) with their positions (num x 2 floats: x, y), one feature
     * each, from host memory onto GPU `device` (popsift_hip_devfeatures_from_host_points): for keypoints and descriptors
     * that come from elsewhere.  The caller owns the result. */
    static FeaturesDev* fromHostPoints(const float* desc, const float* xy, int num, int device = 0);

    /* extension: (x, y, x', y') of each pair -- the positions of the features behind descriptor l of this set and
     * descriptor r of `other` -- gathered on the GPU (popsift_hip_pair_points): the input of popsift::Verifier
     * (popsift/verify.h).  The pairs of a byte match (FeaturesDevBytes::matchPairs) index the float sets the bytes came
     * from, so they go through the same call on those. */
    std::vector<float> pairPoints(FeaturesDev* other, const std::vector<Pair>& pairs);

    /* DEVICE pointers */
    Feature*    getFeatures();
    Descriptor* getDescriptors();
    int*        getReverseMap();

    int                      getDevice() const;
    popsift_hip_devfeatures* getHandle() { return _set; }

    /* extension: this set's descriptors as bytes, quantized on its GPU (the rule of Config::ByteDescriptors /
     * popsift_hip_fetch_item_u8), with a copy of the reverse map.  The caller owns the result; null for an unset object. */
    FeaturesDevBytes* toBytes() const;
};

/*
 * Extension: a device-resident set of byte descriptors (popsift_hip_bytefeatures) -- a quarter of FeaturesDev's memory --
 * and its exact matcher: squared distances are integers, ties go to the lower index, no float summation order is involved.
 * matchAndGet / matchPairs mirror FeaturesDev's; maxDist2 is in byte units squared.
 */
class FeaturesDevBytes {
    popsift_hip_bytefeatures* _set;

    FeaturesDevBytes(const FeaturesDevBytes&);
    FeaturesDevBytes& operator=(const FeaturesDevBytes&);

public:
    typedef FeaturesDev::Match        Match;
    typedef FeaturesDev::MatchOptions MatchOptions;
    typedef FeaturesDev::Pair         Pair;

    /* takes ownership of a set made by the C ABI */
    explicit FeaturesDevBytes(popsift_hip_bytefeatures* adopt) : _set(adopt) {}
    /* num_ori x 128 bytes of host memory onto GPU `device` */
    FeaturesDevBytes(const unsigned char* desc, int num_ori, int device = 0);
    ~FeaturesDevBytes();

    int getDescriptorCount() const;
    int getDevice() const;
    popsift_hip_bytefeatures* getHandle() { return _set; }

    std::vector<Match> matchAndGet(FeaturesDevBytes* other);
    std::vector<Pair>  matchPairs(FeaturesDevBytes* other, const MatchOptions& opts);
    std::vector<Pair>  matchPairs(FeaturesDevBytes* other) { return matchPairs(other, MatchOptions()); }
};

/*
 * Extension: byte sets end to end on one GPU (popsift_hip_gallery), matched against one query set in one pass: what
 * query->matchPairs(member) returns for every member, from a fixed number of kernel launches and one download instead of
 * a loop of calls.  add() copies the set's bytes on the device; the set may be deleted afterwards.  Pair indices are
 * those of the sets the members came from.  One call at a time per gallery; the query is only read.  A member added as a
 * FeaturesDev brings the positions of its features along, and pairPoints() turns the pair lists into the points of
 * Verifier::ransacMany (popsift/verify.h): every gallery image verified in one call.
 */
class Gallery {
    popsift_hip_gallery* _gallery;

    Gallery(const Gallery&);
    Gallery& operator=(const Gallery&);

public:
    typedef FeaturesDev::MatchOptions MatchOptions;
    typedef FeaturesDev::Pair         Pair;

    explicit Gallery(int device = 0);
    ~Gallery();

    /* the new member's index: 0, 1, ... */
    int add(FeaturesDevBytes* member);
    /* a member from a float set (popsift_hip_gallery_add_set): the bytes of member->toBytes() and, for pairPoints, the
     * positions of the features behind its descriptors */
    int add(FeaturesDev* member);
    /* members */
    int size() const;
    popsift_hip_gallery* getHandle() { return _gallery; }

    /* one pair list per member, each as FeaturesDevBytes::matchPairs(member, opts) returns it */
    std::vector<std::vector<Pair>> matchPairs(FeaturesDevBytes* query, const MatchOptions& opts);
    std::vector<std::vector<Pair>> matchPairs(FeaturesDevBytes* query) { return matchPairs(query, MatchOptions()); }
    /* the lengths of those lists alone: no pair is downloaded */
    std::vector<int> counts(FeaturesDevBytes* query, const MatchOptions& opts);

    /* (x, y, x', y') of every pair of matchPairs' lists, list after list, and the lists' offsets (size() + 1, from 0)
     * into them (popsift_hip_gallery_pair_points): the input of Verifier::ransacMany.  query is the float set the query
     * bytes came from; every member with a pair was added as a FeaturesDev. */
    std::vector<float> pairPoints(FeaturesDev* query, const std::vector<std::vector<Pair>>& pairs, std::vector<int>& offsets);

    /* Members against members (popsift_hip_match_pairs_links): a link is an ordered pair of member indices, left image a
     * and right image b; any list of them, a == b and repeats included. */
    struct Link {
        int a, b;
    };
    /* every a < b of n members, a-major: exhaustive matching */
    static std::vector<Link> allLinks(int n);
    /* (a, a + 1 .. a + k) for every member a of a sequence of n */
    static std::vector<Link> sequentialLinks(int n, int k);
    /* one pair list per link, each as memberA->matchPairs(memberB, opts) returns it for the sets the members came from */
    std::vector<std::vector<Pair>> matchPairs(const std::vector<Link>& links, const MatchOptions& opts);
    std::vector<std::vector<Pair>> matchPairs(const std::vector<Link>& links) { return matchPairs(links, MatchOptions()); }
    /* (x, y, x', y') of every pair of those lists, list after list, and the lists' offsets (links.size() + 1, from 0)
     * into them (popsift_hip_gallery_link_points): the input of Verifier::ransacMany.  Both positions are the members'
     * own: every member of a link with a pair was added as a FeaturesDev. */
    std::vector<float> pairPoints(const std::vector<Link>& links, const std::vector<std::vector<Pair>>& pairs, std::vector<int>& offsets);
};

}  // namespace popsift
