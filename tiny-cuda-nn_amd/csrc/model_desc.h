// model_desc.h -- description of a model (encoding + optional fully fused network): what the JSON configuration asks for, resolved
// into the metadata the kernels take, plus parameter initialisation.  Mirrors the reference's
//   include/tiny-cuda-nn/config.h:46-63, network_with_input_encoding.h:55-130, grid.h:673-737/1725-1852, src/network.cu:51-138
// for the HashGrid + FullyFusedMLP hot path only.
#pragma once
#include <string>

#include "../../include/tiny-cuda-nn/json_mini.h"
#include "adam_device.h"
#include "elementwise_kernels.h"
#include "grid_kernels.h"
#include "mlp_kernels.h"

namespace tcnn_hip {

struct EncodingDesc {
	bool is_grid = false;
	// grid (grid.h:673-737)
	GridMeta grid = {};
	uint32_t log2_hashmap_size = 19, base_resolution = 16;
	float per_level_scale = 2.0f;
	// identity (identity.h:88-93)
	float id_scale = 1.0f, id_offset = 0.0f;
	// one-blob (oneblob.h:168-178): n_bins outputs per input dimension
	bool is_oneblob = false;
	uint32_t n_bins = 0;
	// frequency (frequency.h:106-111): sin and cos of n_frequencies octaves per input dimension
	bool is_frequency = false;
	uint32_t n_frequencies = 0;
	uint32_t n_dims = 0;
	uint32_t n_output_dims = 0;  // before padding
	uint32_t n_params = 0;
	uint32_t padded_output_width = 0;

	uint32_t required_output_alignment() const { return is_grid ? grid.n_feat : 1u; }  // grid.h:1066-1068
	void set_alignment(uint32_t alignment);  // encoding.h:70-72
	Json hyperparams() const;
};

struct NetworkDesc {
	MlpMeta mlp = {};
	uint32_t n_output_dims = 0;
	uint32_t n_hidden_layers = 0;
	std::string otype;
	Json hyperparams() const;  // fully_fused_mlp.h:139-147
};

// A NetworkWithInputEncoding (network_with_input_encoding.h:40-130) or a bare encoding.
struct Model {
	uint32_t n_input_dims = 0;
	EncodingDesc enc;
	bool has_network = false;
	NetworkDesc net;
	std::string hyper_json;

	size_t n_mlp_params() const { return has_network ? net.mlp.n_params() : 0; }
	size_t n_params() const { return n_mlp_params() + enc.n_params; }  // network first, then encoding (:115-122)
	uint32_t padded_output_width() const { return has_network ? net.mlp.padded_out : enc.padded_output_width; }
	uint32_t output_width() const { return has_network ? net.n_output_dims : enc.padded_output_width; }
	std::string name() const { return has_network ? "NetworkWithInputEncoding" : (enc.is_grid ? "GridEncoding" : (enc.is_oneblob ? "OneBlobEncoding" : (enc.is_frequency ? "FrequencyEncoding" : "IdentityEncoding"))); }

	void finish();  // fills hyper_json
	// network_with_input_encoding.h:124-130 + fully_fused_mlp.cu:868-893 + grid.h:1076-1079
	void initialize_params(hipStream_t stream, Pcg32& rng, float* params_full_precision, float scale) const;
};

EncodingDesc create_encoding_desc(uint32_t n_dims, const Json& enc, uint32_t alignment);  // encoding.cu:131-145
Model make_nwie(uint32_t n_input_dims, uint32_t n_output_dims, const Json& encoding, const Json& network);
const char* loss_name(LossType loss);  // loss.cu:57-65
LossType string_to_loss(const std::string& s);
void parse_adam(AdamHyper& h, const Json& p);  // adam.h:221-281

}  // namespace tcnn_hip
