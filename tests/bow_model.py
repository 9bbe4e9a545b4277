"""ORBVocabulary::transform by the book, written from the reference's text (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h :1126-1194 the
loop over the features, :1217-1259 the descent of one feature; BowVector.cpp :34-46 addWeight, :50-58 addIfNotExist, :62-84 normalize;
FeatureVector::addFeature; FORB::distance FORB.cpp:81-101), not from oracle/orc_match.c or the kernels of eorb_slam_amd/csrc/match.hip.

The descent counts bits with a 256-entry table and takes the FIRST minimum among a node's children (`d < best_d`, :1244).  The BowVector
is a dict walked in ascending word id, which is std::map's order; a TF / TF_IDF value is built by repeated `+= w` in feature order
(addWeight), an IDF / BINARY value is the first one seen (addIfNotExist); without a norm the TF / TF_IDF values are divided by the
number of words (:1164-1170); the L1 / L2 norm is summed in ascending word order.  The FeatureVector is a dict from node to the list
of feature indices in push_back order.  Every value is a Python float, an IEEE double with one rounding per operation, so the
comparison with the oracle and the kernels is bit for bit (view(np.uint64)).

One defined choice where the reference reads an uninitialised value: when a ragged tree ends a branch on a leaf above level
L - levelsup, the descent never reaches the nid level and `NodeId nid` (:1151) is never written (:1251).  Model, oracle and kernel
answer node 0 there, the value the reference itself gives when L - levelsup <= 0 (:1227).

The weight of a word is the vocabulary's stored weight whatever the weighting (setNodeWeights stores 1 for TF / BINARY); a word with
weight 0 is stopped (`if(w > 0)`, :1157).

transform() returns the five outputs of oracle.bow_transform and a probe: what the scene exercised (tests/bow_scenes.py asserts the
condition each scene exists for).  `wrong=` takes a named wrong variant (WRONG below) that changes one rule;
tests/test_oracle_bow_model.py holds the oracle to the model and shows that a named scene tells every variant from the rule;
tests/test_gpu_bow_model.py holds the kernels."""
import math

import numpy as np

WRONG = {
    "tie_last_child": "the last minimum wins a descent tie",
    "nid_level_off_by_one": "the node is taken one level above level L - levelsup",
    "short_leaf_nid_is_leaf": "a leaf above the nid level answers itself instead of 0",
    "stopped_kept_in_fv": "stopped words stay in the feature vector",
    "idf_accumulates": "IDF / BINARY values accumulate per occurrence",
    "count_times_w": "count x w for the repeated addition",
    "norm_in_feature_order": "the norm summed in first-occurrence order",
    "tf_unnormalised_not_divided": "no division by the word count",
    "fv_keyed_by_word": "the feature vector keyed by word",
}

POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def sort_size(n):
    """P, the power of two >= max(n, 64) that bow_assemble_kernel sorts, and the register class M of block_bitonic_sort_regs"""
    P = 64
    while P < n:
        P *= 2
    return P, max(1, P // 1024)


def descend(voc, desc, levelsup, wrong=None):
    """TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) :1217-1259 for every row of desc (its first 32 bytes).
    Returns per feature (leaf node, nid) and the probe's descent part.  Features with equal bytes share one descent."""
    child_off, child_ids, node_desc = voc["child_off"], voc["child_ids"], np.asarray(voc["node_desc"], np.uint8)
    nid_level = int(voc["L"]) - levelsup                                     # :1226
    if wrong == "nid_level_off_by_one":
        nid_level -= 1
    out, seen = [], {}
    probe = dict(tie=False, short_leaf=False, widest=0)
    for row in np.asarray(desc, np.uint8):
        feature = row[:32]
        key = feature.tobytes()
        if key not in seen:
            nid = 0                                                          # :1227, and the defined choice for a short leaf
            final_id, current_level = 0, 0
            tie, widest = False, 0
            while True:
                current_level += 1
                nodes = child_ids[child_off[final_id]:child_off[final_id + 1]]
                d = POP8[node_desc[nodes] ^ feature].sum(axis=1)
                best = int(d.min())
                at = np.flatnonzero(d == best)
                tie = tie or len(at) > 1
                widest = max(widest, len(nodes))
                final_id = int(nodes[at[-1] if wrong == "tie_last_child" else at[0]])
                if current_level == nid_level:                               # :1251
                    nid = final_id
                if child_off[final_id + 1] == child_off[final_id]:           # isLeaf() :1254
                    break
            short = 0 < nid_level and current_level < nid_level
            if short and wrong == "short_leaf_nid_is_leaf":
                nid = final_id
            seen[key] = (final_id, nid, tie, short, widest)
        final_id, nid, tie, short, widest = seen[key]
        probe["tie"] |= tie; probe["short_leaf"] |= short; probe["widest"] = max(probe["widest"], widest)
        out.append((final_id, nid))
    return out, probe


def assemble(voc, walked, weighting, norm, wrong=None):
    """TemplatedVocabulary::transform(features, v, fv, levelsup) :1126-1194 given every feature's (leaf, nid)"""
    word_id, weight = voc["word_id"], voc["weight"]
    n = len(walked)
    v, fv, count, first_w = {}, {}, {}, {}
    word_of, node_of = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    accumulate = weighting in (0, 1) or wrong == "idf_accumulates"           # TF_IDF, TF :1145
    m = 0
    for i_feature, (leaf, nid) in enumerate(walked):
        wid, w = int(word_id[leaf]), float(weight[leaf])
        if w > 0:                                                            # not stopped :1157, :1185
            m += 1
            word_of[i_feature], node_of[i_feature] = wid, nid
            count[wid] = count.get(wid, 0) + 1
            if wid not in v:
                v[wid] = first_w[wid] = w
            elif accumulate:
                v[wid] = v[wid] + w                                          # addWeight: vit->second += v
            fv.setdefault(wid if wrong == "fv_keyed_by_word" else nid, []).append(i_feature)
        elif wrong == "stopped_kept_in_fv":
            fv.setdefault(nid, []).append(i_feature)
    if wrong == "count_times_w" and accumulate:
        for wid in v:
            v[wid] = count[wid] * first_w[wid]
    order = list(v) if wrong == "norm_in_feature_order" else sorted(v)
    if weighting in (0, 1) and v and norm == 0 and wrong != "tf_unnormalised_not_divided":
        nd = float(len(v))                                                   # :1164-1170
        for wid in v:
            v[wid] = v[wid] / nd
    if norm != 0:                                                            # BowVector::normalize
        s = 0.0
        if norm == 1:
            for wid in order:
                s += abs(v[wid])
        else:
            for wid in order:
                s += v[wid] * v[wid]
            s = math.sqrt(s)
        if s > 0.0:
            for wid in v:
                v[wid] = v[wid] / s
    words = sorted(v)
    nodes = sorted(fv)
    fv_off = np.zeros(len(nodes) + 1, np.int32)
    fv_off[1:] = np.cumsum([len(fv[k]) for k in nodes])
    fv_idx = np.array([i for k in nodes for i in fv[k]], np.int32).reshape(-1)
    P, M = sort_size(n)
    probe = dict(n=n, m=m, words=len(words), nodes=len(nodes), longest_word_run=max(count.values()) if count else 0,
                 longest_node_run=max((len(x) for x in fv.values()), default=0), P=P, M=M)
    return (np.array(words, np.uint32), np.array([v[k] for k in words], np.float64), (np.array(nodes, np.uint32), fv_off, fv_idx),
            word_of, node_of, probe)


def transform(voc, desc, levelsup=4, weighting=0, norm=1, wrong=None, walked=None):
    """Returns (bow_word, bow_val, (fv_node, fv_off, fv_idx), word_of, node_of, probe).  walked: the result of descend() for the same
    vocabulary, descriptors and levelsup, when several (weighting, norm) pairs share it."""
    if len(voc["child_off"]) - 1 <= 1 or len(desc) == 0:                     # empty() :1134
        z = np.zeros(0, np.int32)
        P, M = sort_size(0)
        return (np.zeros(0, np.uint32), np.zeros(0, np.float64), (np.zeros(0, np.uint32), np.zeros(1, np.int32), z),
                np.zeros(len(desc), np.int32), np.zeros(len(desc), np.int32),
                dict(n=len(desc), m=0, words=0, nodes=0, longest_word_run=0, longest_node_run=0, P=P, M=M, tie=False, short_leaf=False, widest=0))
    if walked is None:
        walked = descend(voc, desc, levelsup, wrong)
    out = assemble(voc, walked[0], weighting, norm, wrong)
    out[5].update(walked[1])
    return out
