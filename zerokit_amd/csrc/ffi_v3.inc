// ffi_v3.inc -- the ffi_rln_v3_* mirror of the zerokit C ABI (/root/reference/rln/src/ffi/ffi_rln_v3.rs:323-1609),
// textually included at the end of ffi.cpp: the V3 objects ARE the V1 objects (same prover, tree, witness, proof
// and values structs); what differs is the constructor set (stateless / tree flavours), the error texts
// (error.rs:104-208) and the wire formats (enum tag + arkworks field order, protocol/serialize.rs:63-714).
//
// Tree flavours: FullMerkleTree, OptimalMerkleTree and PmTree all map to the one HBM-resident tree of merkle.hip
// (identical roots and proofs, rln/tests/poseidon_tree.rs:14-41); the pm-tree constructor that takes a config file
// shares FFI_RLN::open_tree and so the durable store of tree_store.h (sled's own on-disk format stays out of scope,
// SURVEY.md section 8f rank 4); `flush` syncs that store's journal and is a no-op for a temporary tree.

namespace {

const char* NO_STATELESS_TREE_ERR = "tree op unsupported on stateless RLN";  // ffi_rln_v3.rs:19

void v3_check_depth(const Prover& P, size_t path_len, size_t index_len) {  // error.rs:168-173
  size_t d = P.graph().tree_depth;
  if (path_len != d)
    throw Error("Field `path_elements` has length " + std::to_string(path_len) + ", but circuit tree_depth is " +
                std::to_string(d));
  if (index_len != d)
    throw Error("Field `identity_path_index` has length " + std::to_string(index_len) +
                ", but circuit tree_depth is " + std::to_string(d));
}
void v3_check_against_graph(const Prover& P, const FFI_RLNWitnessInput& w) {  // witness.rs:1110-1151
  v3_check_depth(P, w.path_elements.size(), w.identity_path_index.size());
  size_t mo = P.graph().max_out;
  if (!w.multi) {
    if (mo != 1) throw Error("Field `message_ids` has length 1, but circuit max_out is " + std::to_string(mo));
    return;
  }
  if (w.message_ids.size() != mo)
    throw Error("Field `message_ids` has length " + std::to_string(w.message_ids.size()) + ", but circuit max_out is " +
                std::to_string(mo));
  if (w.selector_used.size() != mo)
    throw Error("Field `selector_used` has length " + std::to_string(w.selector_used.size()) +
                ", but circuit max_out is " + std::to_string(mo));
}
// run f and re-label the V1 error prefixes (error.rs:57 / :175-178)
template <class F>
auto v3_relabel(F&& f) -> decltype(f()) {
  try {
    return f();
  } catch (const Error& e) {
    std::string m = e.what();
    const std::string a = "Error calculating witness: ", b = "Error producing proof: ";
    if (m.compare(0, a.size(), a) == 0) throw Error("Witness calculation error: " + m.substr(a.size()));
    if (m.compare(0, b.size(), b) == 0) throw Error("Synthesis error: " + m.substr(b.size()));
    throw;
  }
}

FFI_RLN* v3_create(bool stateless, size_t depth, const Vec_uint8_t* zkey, const Vec_uint8_t* graph,
                   const TreeConfig* tcfg = nullptr) {
  std::vector<uint8_t> z, g;
  if (zkey && graph) {
    z.assign(zkey->ptr, zkey->ptr + zkey->len);
    g.assign(graph->ptr, graph->ptr + graph->len);
  } else {  // RLNBuilder defaults: the embedded depth-20 single message-id circuit (public.rs:960-996)
    std::string dir = resource_dir(20);
    z = read_file(dir + "/rln_final.arkzkey");
    g = read_file(dir + "/graph.bin");
  }
  require_gpu();
  std::unique_ptr<FFI_RLN> r(new FFI_RLN);
  // "window_bits" / "max_batch" / "devices" of the config file; graph_from_raw(.., None, None)
  r->make_prover(z.data(), z.size(), g.data(), g.size(), tcfg ? *tcfg : TreeConfig());
  r->stateless = stateless;
  if (!stateless) {
    if (tcfg) r->open_tree(depth, *tcfg); else r->new_tree(depth);
  }
  return r.release();
}
FFI_RLN* v3_default(bool stateless) {  // the *_default constructors return a bare Box: NULL when no device
  try {
    return v3_create(stateless, 20, nullptr, nullptr);
  } catch (const std::exception& e) {
    fprintf(stderr, "librln: %s\n", e.what());
    return nullptr;
  }
}

}  // namespace

extern "C" {

#define V3RLN(r) (*(FFI_RLN*)*(r))
#define V3_TREE_GUARD(r) \
  if (V3RLN(r).stateless) return {false, make_str(NO_STATELESS_TREE_ERR)}

// ================================================================================ constructors (:323-504)
FFI_RLNV3_t* ffi_rln_v3_new_stateless_default(void) { return (FFI_RLNV3_t*)v3_default(true); }
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_stateless(const Vec_uint8_t* zkey_data, const Vec_uint8_t* graph_data) {
  return guard_ptr<CResult_FFI_RLNV3_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3_t* { return (FFI_RLNV3_t*)v3_create(true, 0, zkey_data, graph_data); });
}
FFI_RLNV3_t* ffi_rln_v3_new_with_full_merkle_tree_default(void) { return (FFI_RLNV3_t*)v3_default(false); }
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_with_full_merkle_tree(size_t tree_depth, const Vec_uint8_t* zkey_data,
                                                                      const Vec_uint8_t* graph_data) {
  return guard_ptr<CResult_FFI_RLNV3_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3_t* { return (FFI_RLNV3_t*)v3_create(false, tree_depth, zkey_data, graph_data); });
}
FFI_RLNV3_t* ffi_rln_v3_new_with_optimal_merkle_tree_default(void) { return (FFI_RLNV3_t*)v3_default(false); }
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_with_optimal_merkle_tree(size_t tree_depth,
                                                                         const Vec_uint8_t* zkey_data,
                                                                         const Vec_uint8_t* graph_data) {
  return ffi_rln_v3_new_with_full_merkle_tree(tree_depth, zkey_data, graph_data);
}
FFI_RLNV3_t* ffi_rln_v3_new_with_pm_tree_default(void) { return (FFI_RLNV3_t*)v3_default(false); }
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_with_pm_tree(size_t tree_depth, const Vec_uint8_t* zkey_data,
                                                             const Vec_uint8_t* graph_data, const char* config_path) {
  return guard_ptr<CResult_FFI_RLNV3_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3_t* {
    TreeConfig tcfg;
    try {
      tcfg = tree_config_from_file(config_path);
    } catch (const Error& e) {  // here the reference returns FromConfigError's own text (ffi_rln_v3.rs:476-483)
      std::string m = e.what();
      const std::string pre = "Configuration error: ";
      throw Error(m.compare(0, pre.size(), pre) == 0 ? m.substr(pre.size()) : m);
    }
    return (FFI_RLNV3_t*)v3_create(false, tree_depth, zkey_data, graph_data, &tcfg);
  });
}
void ffi_rln_v3_free(FFI_RLNV3_t* rln) { delete (FFI_RLN*)rln; }

// ================================================================================ proofs (:506-604)
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_rln_v3_generate_proof(FFI_RLNV3_t* const* rln,
                                                                FFI_RLNV3WitnessInput_t* const* witness) {
  return guard_ptr<CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3Proof_t* {
    FFI_RLN& r = V3RLN(rln);
    FFI_RLNWitnessInput* w = (FFI_RLNWitnessInput*)*witness;
    v3_check_against_graph(*r.prover, *w);
    return (FFI_RLNV3Proof_t*)v3_relabel([&]() { return prove_one(r, w, nullptr); });
  });
}
/* EXT: deterministic blinding, as ffi_generate_rln_proof_with_rs */
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_rln_v3_generate_proof_with_rs(FFI_RLNV3_t* const* rln,
                                                                        FFI_RLNV3WitnessInput_t* const* witness,
                                                                        const CFr_t* rr, const CFr_t* ss) {
  return guard_ptr<CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3Proof_t* {
    FFI_RLN& r = V3RLN(rln);
    FFI_RLNWitnessInput* w = (FFI_RLNWitnessInput*)*witness;
    v3_check_against_graph(*r.prover, *w);
    CFr rs[2] = {R(rr), R(ss)};
    return (FFI_RLNV3Proof_t*)v3_relabel([&]() { return prove_one(r, w, rs); });
  });
}
CBoolResult_t ffi_rln_v3_verify(FFI_RLNV3_t* const* rln, FFI_RLNV3Proof_t* const* proof, const CFr_t* x) {
  const FFI_RLNProof& pr = *(FFI_RLNProof*)*proof;
  if (cfr_cmp(R(x), pr.values.x) != 0) return {false, no_err()};  // :529-534: plain false, no error text
  try {
    bool ok = v3_relabel([&]() { return verify_zk(V3RLN(rln), pr); });
    return {ok, no_err()};
  } catch (const std::exception& e) {
    return {false, make_str(e.what())};
  }
}
CBoolResult_t ffi_rln_v3_verify_with_roots(FFI_RLNV3_t* const* rln, FFI_RLNV3Proof_t* const* proof,
                                           const Vec_CFr_t* roots, const CFr_t* x) {
  return guard_bool([&]() {  // public.rs:938-955: root, then signal, then proof
    const FFI_RLNProof& pr = *(FFI_RLNProof*)*proof;
    if (roots && roots->len) {
      bool found = false;
      for (size_t i = 0; i < roots->len; i++) found |= cfr_cmp(((const CFr*)roots->ptr)[i], pr.values.root) == 0;
      if (!found) throw Error("Expected one of the provided roots");
    }
    if (cfr_cmp(R(x), pr.values.x) != 0) throw Error("Signal value does not match");
    if (!v3_relabel([&]() { return verify_zk(V3RLN(rln), pr); })) throw Error("Invalid proof provided");
    return true;
  });
}
CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t ffi_rln_v3_generate_partial_proof(
    FFI_RLNV3_t* const* rln, FFI_RLNV3PartialWitnessInput_t* const* partial_witness) {
  return guard_ptr<CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3PartialProof_t* {
    FFI_RLN& r = V3RLN(rln);
    const FFI_RLNPartialWitnessInput& pw = *(FFI_RLNPartialWitnessInput*)*partial_witness;
    v3_check_depth(*r.prover, pw.path_elements.size(), pw.identity_path_index.size());
    return (FFI_RLNV3PartialProof_t*)v3_relabel([&]() { return prove_partial(r, pw); });
  });
}
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_rln_v3_finish_proof(FFI_RLNV3_t* const* rln,
                                                              FFI_RLNV3PartialProof_t* const* partial,
                                                              FFI_RLNV3WitnessInput_t* const* witness) {
  return guard_ptr<CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3Proof_t* {
    FFI_RLN& r = V3RLN(rln);
    FFI_RLNWitnessInput& w = *(FFI_RLNWitnessInput*)*witness;
    v3_check_against_graph(*r.prover, w);
    return (FFI_RLNV3Proof_t*)v3_relabel(
        [&]() { return finish_one(r, *(FFI_RLNPartialProof*)*partial, w, random_fr(), random_fr()); });
  });
}

// ================================================================================ witness input (:612-862)
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_rln_v3_witness_input_new_single(
    const CFr_t* identity_secret, const CFr_t* user_message_limit, const CFr_t* message_id,
    const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index, const CFr_t* x,
    const CFr_t* external_nullifier) {
  return guard_ptr<CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3WitnessInput_t* {
    std::unique_ptr<FFI_RLNWitnessInput> w(new FFI_RLNWitnessInput);
    w->identity_secret = R(identity_secret);
    w->user_message_limit = R(user_message_limit);
    w->message_id = R(message_id);
    w->path_elements.assign((const CFr*)path_elements->ptr, (const CFr*)path_elements->ptr + path_elements->len);
    w->identity_path_index.assign(identity_path_index->ptr, identity_path_index->ptr + identity_path_index->len);
    w->x = R(x);
    w->external_nullifier = R(external_nullifier);
    v3_validate_witness(*w);
    return (FFI_RLNV3WitnessInput_t*)w.release();
  });
}
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_rln_v3_witness_input_new_multi(
    const CFr_t* identity_secret, const CFr_t* user_message_limit, const Vec_CFr_t* message_ids,
    const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index, const CFr_t* x,
    const CFr_t* external_nullifier, const Vec_bool_t* selector_used) {
  return guard_ptr<CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3WitnessInput_t* {
    std::unique_ptr<FFI_RLNWitnessInput> w(new FFI_RLNWitnessInput);
    w->multi = true;
    w->identity_secret = R(identity_secret);
    w->user_message_limit = R(user_message_limit);
    w->message_id = cfr_from_u64(0);
    w->message_ids.assign((const CFr*)message_ids->ptr, (const CFr*)message_ids->ptr + message_ids->len);
    w->path_elements.assign((const CFr*)path_elements->ptr, (const CFr*)path_elements->ptr + path_elements->len);
    w->identity_path_index.assign(identity_path_index->ptr, identity_path_index->ptr + identity_path_index->len);
    w->x = R(x);
    w->external_nullifier = R(external_nullifier);
    for (size_t i = 0; i < selector_used->len; i++) w->selector_used.push_back(selector_used->ptr[i] ? 1 : 0);
    v3_validate_witness(*w);
    return (FFI_RLNV3WitnessInput_t*)w.release();
  });
}
#define V3W(w) (*(FFI_RLNWitnessInput*)*(w))
CFr_t* ffi_rln_v3_witness_input_get_identity_secret(FFI_RLNV3WitnessInput_t* const* w) { return box_cfr(V3W(w).identity_secret); }
CFr_t* ffi_rln_v3_witness_input_get_user_message_limit(FFI_RLNV3WitnessInput_t* const* w) { return box_cfr(V3W(w).user_message_limit); }
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_witness_input_get_message_id(FFI_RLNV3WitnessInput_t* const* w) {
  if (V3W(w).multi) return {nullptr, make_str("witness is Multi; use get_message_ids")};
  return {box_cfr(V3W(w).message_id), no_err()};
}
CResult_Vec_CFr_Vec_uint8_t ffi_rln_v3_witness_input_get_message_ids(FFI_RLNV3WitnessInput_t* const* w) {
  if (!V3W(w).multi) return {Vec_CFr_t{nullptr, 0, 0}, make_str("witness is Single; use get_message_id")};
  return {make_vec_cfr(V3W(w).message_ids), no_err()};
}
Vec_CFr_t ffi_rln_v3_witness_input_get_path_elements(FFI_RLNV3WitnessInput_t* const* w) { return make_vec_cfr(V3W(w).path_elements); }
Vec_uint8_t ffi_rln_v3_witness_input_get_identity_path_index(FFI_RLNV3WitnessInput_t* const* w) { return make_bytes(V3W(w).identity_path_index); }
CFr_t* ffi_rln_v3_witness_input_get_x(FFI_RLNV3WitnessInput_t* const* w) { return box_cfr(V3W(w).x); }
CFr_t* ffi_rln_v3_witness_input_get_external_nullifier(FFI_RLNV3WitnessInput_t* const* w) { return box_cfr(V3W(w).external_nullifier); }
CResult_Vec_bool_Vec_uint8_t ffi_rln_v3_witness_input_get_selector_used(FFI_RLNV3WitnessInput_t* const* w) {
  if (!V3W(w).multi) return {Vec_bool_t{nullptr, 0, 0}, make_str("witness is Single; selector_used is Multi-only")};
  return {make_vec_bool(V3W(w).selector_used), no_err()};
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_witness_to_bytes_le(FFI_RLNV3WitnessInput_t* const* w) {
  return guard_bytes([&]() { return v3_witness_bytes(V3W(w), false); });
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_witness_to_bytes_be(FFI_RLNV3WitnessInput_t* const* w) {
  return guard_bytes([&]() { return v3_witness_bytes(V3W(w), true); });
}
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_witness(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3WitnessInput_t* { return (FFI_RLNV3WitnessInput_t*)v3_witness_from(bytes, false); });
}
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_bytes_be_to_rln_v3_witness(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3WitnessInput_t* { return (FFI_RLNV3WitnessInput_t*)v3_witness_from(bytes, true); });
}
void ffi_rln_v3_witness_input_free(FFI_RLNV3WitnessInput_t* w) { delete (FFI_RLNWitnessInput*)w; }

// ================================================================================ partial witness (:864-1009)
CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t ffi_rln_v3_partial_witness_input_new(
    const CFr_t* identity_secret, const CFr_t* user_message_limit, const Vec_CFr_t* path_elements,
    const Vec_uint8_t* identity_path_index) {
  return guard_ptr<CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3PartialWitnessInput_t* {
    std::unique_ptr<FFI_RLNPartialWitnessInput> w(new FFI_RLNPartialWitnessInput);
    w->identity_secret = R(identity_secret);
    w->user_message_limit = R(user_message_limit);
    w->path_elements.assign((const CFr*)path_elements->ptr, (const CFr*)path_elements->ptr + path_elements->len);
    w->identity_path_index.assign(identity_path_index->ptr, identity_path_index->ptr + identity_path_index->len);
    v3_validate_common(w->user_message_limit, w->path_elements.size(), w->identity_path_index.size());
    return (FFI_RLNV3PartialWitnessInput_t*)w.release();
  });
}
#define V3PW(w) (*(FFI_RLNPartialWitnessInput*)*(w))
CFr_t* ffi_rln_v3_partial_witness_input_get_identity_secret(FFI_RLNV3PartialWitnessInput_t* const* w) { return box_cfr(V3PW(w).identity_secret); }
CFr_t* ffi_rln_v3_partial_witness_input_get_user_message_limit(FFI_RLNV3PartialWitnessInput_t* const* w) { return box_cfr(V3PW(w).user_message_limit); }
Vec_CFr_t ffi_rln_v3_partial_witness_input_get_path_elements(FFI_RLNV3PartialWitnessInput_t* const* w) { return make_vec_cfr(V3PW(w).path_elements); }
Vec_uint8_t ffi_rln_v3_partial_witness_input_get_identity_path_index(FFI_RLNV3PartialWitnessInput_t* const* w) { return make_bytes(V3PW(w).identity_path_index); }
FFI_RLNV3PartialWitnessInput_t* ffi_rln_v3_witness_to_partial_witness(FFI_RLNV3WitnessInput_t* const* w) {
  return (FFI_RLNV3PartialWitnessInput_t*)ffi_rln_witness_to_partial_witness((FFI_RLNWitnessInput_t* const*)w);
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_partial_witness_to_bytes_le(FFI_RLNV3PartialWitnessInput_t* const* w) {
  return guard_bytes([&]() { return v3_partial_witness_bytes(V3PW(w), false); });
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_partial_witness_to_bytes_be(FFI_RLNV3PartialWitnessInput_t* const* w) {
  return guard_bytes([&]() { return v3_partial_witness_bytes(V3PW(w), true); });
}
CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_partial_witness(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3PartialWitnessInput_t* {
    return (FFI_RLNV3PartialWitnessInput_t*)v3_partial_witness_from(bytes, false);
  });
}
CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t ffi_bytes_be_to_rln_v3_partial_witness(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t>([&]() -> FFI_RLNV3PartialWitnessInput_t* {
    return (FFI_RLNV3PartialWitnessInput_t*)v3_partial_witness_from(bytes, true);
  });
}
void ffi_rln_v3_partial_witness_input_free(FFI_RLNV3PartialWitnessInput_t* w) { delete (FFI_RLNPartialWitnessInput*)w; }

// ================================================================================ proof objects (:1011-1137)
FFI_RLNV3ProofValues_t* ffi_rln_v3_proof_get_values(FFI_RLNV3Proof_t* const* proof) {
  return (FFI_RLNV3ProofValues_t*)new FFI_RLNProofValues(((FFI_RLNProof*)*proof)->values);
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_to_bytes_le(FFI_RLNV3Proof_t* const* proof) {
  return guard_bytes([&]() { return v3_proof_bytes(*(FFI_RLNProof*)*proof, false); });
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_to_bytes_mixed(FFI_RLNV3Proof_t* const* proof) {
  return guard_bytes([&]() { return v3_proof_bytes(*(FFI_RLNProof*)*proof, true); });
}
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_proof(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3Proof_t* { return (FFI_RLNV3Proof_t*)v3_proof_from(bytes, false); });
}
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_bytes_mixed_to_rln_v3_proof(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3Proof_t* { return (FFI_RLNV3Proof_t*)v3_proof_from(bytes, true); });
}
void ffi_rln_v3_proof_free(FFI_RLNV3Proof_t* proof) { delete (FFI_RLNProof*)proof; }
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_partial_proof_to_bytes_le(FFI_RLNV3PartialProof_t* const* partial) {
  return guard_bytes([&]() { return v3_partial_proof_bytes(*(FFI_RLNPartialProof*)*partial); });
}
CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_partial_proof(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3PartialProof_t* { return (FFI_RLNV3PartialProof_t*)v3_partial_proof_from(bytes); });
}
void ffi_rln_v3_partial_proof_free(FFI_RLNV3PartialProof_t* partial) { delete (FFI_RLNPartialProof*)partial; }

// ================================================================================ proof values (:1139-1321)
#define V3PV(p) (*(FFI_RLNProofValues*)*(p))
CFr_t* ffi_rln_v3_proof_values_get_root(FFI_RLNV3ProofValues_t* const* pv) { return box_cfr(V3PV(pv).root); }
CFr_t* ffi_rln_v3_proof_values_get_x(FFI_RLNV3ProofValues_t* const* pv) { return box_cfr(V3PV(pv).x); }
CFr_t* ffi_rln_v3_proof_values_get_external_nullifier(FFI_RLNV3ProofValues_t* const* pv) { return box_cfr(V3PV(pv).external_nullifier); }
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_proof_values_get_y(FFI_RLNV3ProofValues_t* const* pv) {
  if (V3PV(pv).multi) return {nullptr, make_str("values are Multi; use get_ys")};
  return {box_cfr(V3PV(pv).y), no_err()};
}
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_proof_values_get_nullifier(FFI_RLNV3ProofValues_t* const* pv) {
  if (V3PV(pv).multi) return {nullptr, make_str("values are Multi; use get_nullifiers")};
  return {box_cfr(V3PV(pv).nullifier), no_err()};
}
CResult_Vec_bool_Vec_uint8_t ffi_rln_v3_proof_values_get_selector_used(FFI_RLNV3ProofValues_t* const* pv) {
  if (!V3PV(pv).multi) return {Vec_bool_t{nullptr, 0, 0}, make_str("values are Single; selector_used is Multi-only")};
  return {make_vec_bool(V3PV(pv).selector_used), no_err()};
}
CResult_Vec_CFr_Vec_uint8_t ffi_rln_v3_proof_values_get_ys(FFI_RLNV3ProofValues_t* const* pv) {
  if (!V3PV(pv).multi) return {Vec_CFr_t{nullptr, 0, 0}, make_str("values are Single; use get_y")};
  return {make_vec_cfr(V3PV(pv).ys), no_err()};
}
CResult_Vec_CFr_Vec_uint8_t ffi_rln_v3_proof_values_get_nullifiers(FFI_RLNV3ProofValues_t* const* pv) {
  if (!V3PV(pv).multi) return {Vec_CFr_t{nullptr, 0, 0}, make_str("values are Single; use get_nullifier")};
  return {make_vec_cfr(V3PV(pv).nullifiers), no_err()};
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_values_to_bytes_le(FFI_RLNV3ProofValues_t* const* pv) {
  return guard_bytes([&]() {
    std::vector<uint8_t> b;
    v3_put_values(b, V3PV(pv), false);
    return b;
  });
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_values_to_bytes_be(FFI_RLNV3ProofValues_t* const* pv) {
  return guard_bytes([&]() {
    std::vector<uint8_t> b;
    v3_put_values(b, V3PV(pv), true);
    return b;
  });
}
static FFI_RLNProofValues* v3_pv_from(const Vec_uint8_t* bytes, bool be) {
  V3Reader c{bytes ? bytes->ptr : nullptr, bytes ? bytes->len : 0, 0, be};
  return new FFI_RLNProofValues(v3_values_from(c));
}
CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_proof_values(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3ProofValues_t* { return (FFI_RLNV3ProofValues_t*)v3_pv_from(bytes, false); });
}
CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t ffi_bytes_be_to_rln_v3_proof_values(const Vec_uint8_t* bytes) {
  return guard_ptr<CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t>(
      [&]() -> FFI_RLNV3ProofValues_t* { return (FFI_RLNV3ProofValues_t*)v3_pv_from(bytes, true); });
}
void ffi_rln_v3_proof_values_free(FFI_RLNV3ProofValues_t* pv) { delete (FFI_RLNProofValues*)pv; }

// ================================================================================ slashing (:1323-1361)
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_compute_id_secret(const CFr_t* share1_x, const CFr_t* share1_y,
                                                         const CFr_t* share2_x, const CFr_t* share2_y) {
  return ffi_compute_id_secret(share1_x, share1_y, share2_x, share2_y);
}
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_recover_id_secret(FFI_RLNV3ProofValues_t* const* pv1,
                                                         FFI_RLNV3ProofValues_t* const* pv2) {
  return guard_ptr<CResult_CFr_ptr_Vec_uint8_t>([&]() -> CFr_t* {  // RecoverSecret impls, proof.rs:973-1140
    const FFI_RLNProofValues &a = V3PV(pv1), &b = V3PV(pv2);
    if (cfr_cmp(a.external_nullifier, b.external_nullifier) != 0) {
      // the cross-mode arm always calls Multi.recover_secret(Single): the multi value is reported first
      const FFI_RLNProofValues& first = (!a.multi && b.multi) ? b : a;
      const FFI_RLNProofValues& second = (!a.multi && b.multi) ? a : b;
      throw Error("External nullifiers mismatch: " + cfr_dec(first.external_nullifier) + " != " +
                  cfr_dec(second.external_nullifier));
    }
    const char* none = "No matching nullifier found across the provided proof values";
    if (!a.multi && !b.multi) {
      if (cfr_cmp(a.nullifier, b.nullifier) != 0) throw Error(none);
      return box_cfr(compute_id_secret(a.x, a.y, b.x, b.y));
    }
    if (a.multi && b.multi) {
      for (size_t i = 0; i < a.nullifiers.size(); i++) {
        if (!a.selector_used[i]) continue;
        for (size_t j = 0; j < b.nullifiers.size(); j++)
          if (b.selector_used[j] && cfr_cmp(a.nullifiers[i], b.nullifiers[j]) == 0)
            return box_cfr(compute_id_secret(a.x, a.ys[i], b.x, b.ys[j]));
      }
      throw Error(none);
    }
    const FFI_RLNProofValues& m = a.multi ? a : b;
    const FFI_RLNProofValues& s = a.multi ? b : a;
    for (size_t i = 0; i < m.nullifiers.size(); i++)
      if (m.selector_used[i] && cfr_cmp(m.nullifiers[i], s.nullifier) == 0)
        return box_cfr(compute_id_secret(m.x, m.ys[i], s.x, s.y));
    throw Error(none);
  });
}

CBoolResult_t ffi_rln_v3_nullifier_log_observe(struct rlnamd_nullifier_log* log, FFI_RLNV3ProofValues_t* const* values,
                                               size_t n, const bool* take, const uint64_t* tags, uint8_t* status,
                                               CFr_t* secrets, uint64_t* first_tag) {   // EXT: the V3 values are the same record
  return guard_bool(
      [&]() { return nullifier_log_observe_values(log, (void* const*)values, n, take, tags, status, secrets, first_tag); });
}

CBoolResult_t ffi_rln_v3_relay_step(FFI_RLNV3_t* const* rln, struct rlnamd_nullifier_log* log, FFI_RLNV3Proof_t* const* proofs,
                                    size_t n, const Vec_uint8_t* signals, const Vec_CFr_t* roots, const uint64_t* tags,
                                    uint8_t* verdict, uint8_t* status, CFr_t* secrets, uint64_t* first_tag) {   // EXT: the V3 proofs are the same record
  return guard_bool([&]() {
    return relay_step_common((void* const*)rln, log, (void* const*)proofs, n, signals, roots, tags, verdict, status, secrets,
                             first_tag);
  });
}
CBoolResult_t ffi_rln_v3_relay_set_epochs(FFI_RLNV3_t* const* rln, struct rlnamd_nullifier_log* log,
                                          const CFr_t* external_nullifiers, size_t k, size_t* removed) {   // EXT: the same entry
  return guard_bool([&]() { return relay_set_epochs_common((void* const*)rln, log, external_nullifiers, k, removed); });
}

// ================================================================================ tree (:1363-1609)
void ffi_rln_v3_merkle_proof_free(FFI_RLNV3MerkleProof_t* proof) { ffi_merkle_proof_free((FFI_MerkleProof_t*)proof); }
CBoolResult_t ffi_rln_v3_delete_leaf(FFI_RLNV3_t** rln, size_t index) {
  V3_TREE_GUARD(rln);
  return ffi_delete_leaf((FFI_RLN_t**)rln, index);
}
CBoolResult_t ffi_rln_v3_set_leaf(FFI_RLNV3_t** rln, size_t index, const CFr_t* leaf) {
  V3_TREE_GUARD(rln);
  return ffi_set_leaf((FFI_RLN_t**)rln, index, leaf);
}
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_get_leaf(FFI_RLNV3_t* const* rln, size_t index) {
  if (V3RLN(rln).stateless) return {nullptr, make_str(NO_STATELESS_TREE_ERR)};
  return ffi_get_leaf((FFI_RLN_t* const*)rln, index);
}
size_t ffi_rln_v3_leaves_set(FFI_RLNV3_t* const* rln) {  // :1425-1427: 0 when stateless
  return V3RLN(rln).stateless ? 0 : ffi_leaves_set((FFI_RLN_t* const*)rln);
}
CBoolResult_t ffi_rln_v3_set_next_leaf(FFI_RLNV3_t** rln, const CFr_t* leaf) {
  V3_TREE_GUARD(rln);
  return ffi_set_next_leaf((FFI_RLN_t**)rln, leaf);
}
CBoolResult_t ffi_rln_v3_set_leaves_from(FFI_RLNV3_t** rln, size_t index, const Vec_CFr_t* leaves) {
  V3_TREE_GUARD(rln);
  return ffi_set_leaves_from((FFI_RLN_t**)rln, index, leaves);
}
CBoolResult_t ffi_rln_v3_init_tree_with_leaves(FFI_RLNV3_t** rln, const Vec_CFr_t* leaves) {
  V3_TREE_GUARD(rln);
  return ffi_init_tree_with_leaves((FFI_RLN_t**)rln, leaves);
}
CBoolResult_t ffi_rln_v3_atomic_operation(FFI_RLNV3_t** rln, size_t index, const Vec_CFr_t* leaves,
                                          const Vec_size_t* indices) {
  V3_TREE_GUARD(rln);
  return ffi_atomic_operation((FFI_RLN_t**)rln, index, leaves, indices);
}
CBoolResult_t ffi_rln_v3_seq_atomic_operation(FFI_RLNV3_t** rln, const Vec_CFr_t* leaves, const Vec_uint8_t* indices) {
  V3_TREE_GUARD(rln);
  return ffi_seq_atomic_operation((FFI_RLN_t**)rln, leaves, indices);
}
CFr_t* ffi_rln_v3_get_root(FFI_RLNV3_t* const* rln) {  // :1531-1534: zero when stateless
  if (V3RLN(rln).stateless) return box_cfr(cfr_from_u64(0));
  return ffi_get_root((FFI_RLN_t* const*)rln);
}
CResult_FFI_RLNV3MerkleProof_ptr_Vec_uint8_t ffi_rln_v3_get_merkle_proof(FFI_RLNV3_t* const* rln, size_t index) {
  if (V3RLN(rln).stateless) return {nullptr, make_str(NO_STATELESS_TREE_ERR)};
  CResult_FFI_MerkleProof_ptr_Vec_uint8_t r = ffi_get_merkle_proof((FFI_RLN_t* const*)rln, index);
  return {(FFI_RLNV3MerkleProof_t*)r.ok, r.err};
}
CBoolResult_t ffi_rln_v3_set_metadata(FFI_RLNV3_t** rln, const Vec_uint8_t* metadata) {
  V3_TREE_GUARD(rln);
  return ffi_set_metadata((FFI_RLN_t**)rln, metadata);
}
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_get_metadata(FFI_RLNV3_t* const* rln) {
  if (V3RLN(rln).stateless) return {Vec_uint8_t{nullptr, 0, 0}, make_str(NO_STATELESS_TREE_ERR)};
  return ffi_get_metadata((FFI_RLN_t* const*)rln);
}
CBoolResult_t ffi_rln_v3_flush(FFI_RLNV3_t** rln) {
  V3_TREE_GUARD(rln);
  return ffi_flush((FFI_RLN_t**)rln);
}

}  // extern "C"
