"""Python mirror of the reference's Nova proof API (/root/reference/src/nova/proof.rs:232-392) over
libvdf_nova.so: `public_params`, `InverseMinRootCircuit.{circuits, eval_and_make_circuits}`,
`NovaVDFProof.{prove_recursively, verify, compress}`.  Every heavy step runs as HIP kernels through
the C ABI of libvdf_hip.so; see include/vdf_nova.h (Nova IVC on the Pallas / Vesta cycle, protocol "vdf-nova-ivc-v1")."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .hip import Context, VdfError, RoundTape, PeriodicRows, _ptr
from .minroot import State, _State, _Fe, nova_lib, EvalMode, MinRootVDF, PallasVDF, VestaVDF, FIELD_FP, FIELD_FQ  # noqa: F401

_vp, _i, _u64, _sz = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
for _name, _res, _args in [
    ("vdf_nova_public_params", _i, [_vp, _u64, C.POINTER(_vp)]),
    ("vdf_nova_public_params_ex", _i, [_vp, _u64, _i, _i, C.POINTER(_vp)]),
    ("vdf_nova_public_params_flags", _i, [_vp, _u64, _i, _i, C.c_uint, C.POINTER(_vp)]),
    ("vdf_nova_public_params_tuned", _i, [_vp, _u64, _i, _i, _vp, C.POINTER(_vp)]),
    ("vdf_nova_tuning_default", None, [_vp]),
    ("vdf_nova_ro_preset", _i, [_i, _vp]),
    ("vdf_nova_public_params_ro", _i, [_vp, _u64, _i, _i, _vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_pp_ro", _i, [_vp, _vp]),
    ("vdf_nova_ro_hash_ro", _i, [_vp, _i, _u64, _vp, _sz, _vp]),
    ("vdf_nova_shape_digest_ro", _i, [_vp, _u64, _i, _i, _vp, _vp]),
    ("vdf_nova_aug_synthesize_ro", _i, [_vp, _i, _u64, _i, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz), _vp, _vp]),
    ("vdf_nova_pp_tuning", _i, [_vp, _vp]),
    ("vdf_nova_pp_setup_ms", _i, [_vp, C.POINTER(C.c_double * 7)]),
    ("vdf_nova_pp_memory", _i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_uint)]),
    ("vdf_nova_pp_free", None, [_vp]),
    ("vdf_nova_pp_sizes", _i, [_vp, _i] + [C.POINTER(_u64)] * 5),
    ("vdf_nova_pp_digest", _i, [_vp, _vp]),
    ("vdf_nova_pp_segment", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_pp_early_rows", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_pp_stencil", _i, [_vp]),
    ("vdf_nova_pp_set_verify_multi", _i, [_vp, _i]),
    ("vdf_nova_pp_verify_multi", _i, [_vp]),
    ("vdf_nova_pp_verify_multi_stats", _i, [_vp, C.POINTER(_u64)]),
    ("vdf_nova_shape_stencil", _i, [_u64, _i, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_eval_and_make_circuits", _i, [_i, _u64, _sz, C.POINTER(_State), C.POINTER(_Fe * 3), C.POINTER(_vp)]),
    ("vdf_nova_circuits_from_checkpoints", _i, [_u64, _u64, _sz, _vp, C.POINTER(_Fe * 3), C.POINTER(_vp)]),
    ("vdf_nova_circuits_materialize", _i, [_vp, _vp, _sz, _sz, _i, _vp]),
    ("vdf_nova_circuits_release", _i, [_vp, _sz, _sz]),
    ("vdf_nova_circuits_memory", _i, [_vp, C.POINTER(_sz), C.POINTER(_u64)]),
    ("vdf_nova_circuit_trace", _i, [_vp, _sz, C.POINTER(_vp)]),
    ("vdf_nova_circuits_host_bytes", _i, [_vp, C.POINTER(_u64)]),
    ("vdf_nova_circuits_forward_begin", _i, [_u64, C.POINTER(_State), C.POINTER(_Fe * 3), C.POINTER(_vp)]),
    ("vdf_nova_circuits_push_trace", _i, [_vp, _vp]),
    ("vdf_nova_circuits_push_checkpoints", _i, [_vp, _u64, _vp]),
    ("vdf_nova_public_params_lanes", _i, [_vp, _u64, _sz, _i, _vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_pp_lanes", _sz, [_vp]),
    ("vdf_nova_shape_digest_lanes", _i, [_vp, _u64, _sz, _i, _vp, _vp]),
    ("vdf_nova_shape_stencil_lanes", _i, [_u64, _sz, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_shape_export_lanes", _i, [_u64, _sz, _i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_aug_synthesize_lanes", _i, [_vp, _u64, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz), _vp, _vp]),
    ("vdf_nova_circuits_lanes_begin", _i, [_u64, _sz, _vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_circuits_push_traces", _i, [_vp, _vp, _sz]),
    ("vdf_nova_circuits_push_checkpoints_lanes", _i, [_vp, _u64, _vp, _sz]),
    ("vdf_nova_circuits_lanes", _sz, [_vp]),
    ("vdf_nova_circuit_lane_states", _i, [_vp, _sz, _sz, C.POINTER(_State), C.POINTER(_State)]),
    ("vdf_nova_eval_and_prove", _i, [_vp, _i, C.POINTER(_State), _sz, C.POINTER(_State), C.POINTER(_vp), _vp]),
    ("vdf_nova_prove_recursively_windowed", _i, [_vp, _vp, _u64, _vp, _sz, C.POINTER(_vp)]),      # z0: `arity` elements
    ("vdf_nova_circuits_len", _sz, [_vp]),
    ("vdf_nova_circuits_upload", _i, [_vp, _vp]),
    ("vdf_nova_circuit_states", _i, [_vp, _sz, C.POINTER(_State), C.POINTER(_State)]),
    ("vdf_nova_circuits_free", None, [_vp]),
    ("vdf_nova_prove_recursively", _i, [_vp, _vp, _u64, _vp, C.POINTER(_vp)]),
    ("vdf_nova_prove_step", _i, [_vp, C.POINTER(_vp), _vp, _sz, _vp]),
    ("vdf_nova_verify", _i, [_vp, _vp, _sz, C.POINTER(_Fe * 3), C.POINTER(_Fe * 3), C.POINTER(_i)]),
    ("vdf_nova_proof_free", None, [_vp]),
    ("vdf_nova_proof_num_steps", _sz, [_vp]),
    ("vdf_nova_proof_instance", _i, [_vp, _i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_proof_witness_ptrs", _i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vdf_nova_proof_zi", _i, [_vp, _vp, _vp]),
    ("vdf_nova_proof_last_step", _i, [_vp, _vp]),
    ("vdf_nova_last_step_ms", _i, [_vp, C.POINTER(C.c_double * 8)]),
    ("vdf_nova_proof_set_kernel_timing", _i, [_vp, _i]),
    ("vdf_nova_proof_kernel_events", _i, [_vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    ("vdf_nova_ro_hash", _i, [_i, _u64, _vp, _sz, _vp]),
    ("vdf_nova_ro_constants", _i, [_i, _vp]),
    ("vdf_nova_ro_hash_batch_eval", _i, [_i, _u64, _vp, _sz, _sz, _i, _vp]),
    ("vdf_nova_ro_block_constants", _i, [_vp, _i, _vp, _vp, C.POINTER(_sz)]),
    ("vdf_nova_ro_hash_batch_eval_ro", _i, [_vp, _i, _u64, _vp, _sz, _sz, _i, _vp]),
    ("vdf_nova_shape_digest", _i, [_u64, _i, _i, _vp, _vp]),
    ("vdf_nova_shape_digest_custom", _i, [_vp, _i, _vp, _vp]),
    ("vdf_nova_shape_export", _i, [_u64, _i, _i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_aug_synthesize", _i, [_i, _u64, _i, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz), _vp, _vp]),
    ("vdf_nova_public_params_custom", _i, [_vp, _vp, _i, C.POINTER(_vp)]),
    ("vdf_nova_prove_step_custom", _i, [_vp, C.POINTER(_vp), _vp, _vp]),
    ("vdf_nova_verify_custom", _i, [_vp, _vp, _sz, _vp, _vp, C.POINTER(_i)]),
    ("vdf_cs_is_witness", _i, [_vp]),
    ("vdf_cs_const", C.c_uint32, [_vp, _vp]),
    ("vdf_cs_add", C.c_uint32, [_vp, C.c_uint32, C.c_uint32]),
    ("vdf_cs_sub", C.c_uint32, [_vp, C.c_uint32, C.c_uint32]),
    ("vdf_cs_scale", C.c_uint32, [_vp, C.c_uint32, _vp]),
    ("vdf_cs_alloc", C.c_uint32, [_vp, _vp]),
    ("vdf_cs_mul", C.c_uint32, [_vp, C.c_uint32, C.c_uint32]),
    ("vdf_cs_enforce", _i, [_vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("vdf_cs_value", _i, [_vp, C.c_uint32, _vp]),
    ("vdf_cs_alloc_from", C.c_uint32, [_vp, C.c_uint32]),
    ("vdf_cs_repeat", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    ("vdf_cs_repeat_lanes", _i, [_vp, _vp, _u64, _sz, _vp, _vp, _vp, _sz, _vp]),
    ("vdf_nova_round_body_record", _i, [_i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_round_tape_eval", _i, [_i, _vp, _u64, _vp, _vp, _vp]),
    ("vdf_nova_walk_body_record", _i, [_i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_walk_tape_eval", _i, [_i, _vp, _vp, _vp, _sz, _u64, _vp, _sz, _sz, _sz, _sz, _u64, _u64, _i, _vp, _vp]),
    ("vdf_nova_round_tape_eval_lanes", _i, [_i, _vp, _u64, _sz, _vp, _vp, _sz, _vp]),
    ("vdf_nova_walk_tape_eval_lanes", _i, [_i, _vp, _sz, _vp, _vp, _sz, _u64, _vp, _sz, _sz, _sz, _sz, _vp, _u64, _i, _vp, _vp]),
    ("vdf_cs_pow", C.c_uint32, [_vp, C.c_uint32, _vp]),
    ("vdf_cs_tab", C.c_uint32, [_vp, _vp, _sz, _sz, _sz]),
    ("vdf_cs_pow_chain", C.c_uint32, [_vp, C.c_uint32, _vp, _sz]),
    ("vdf_nova_pow_chain_exponent", _i, [_vp, _sz, _vp, C.POINTER(C.c_uint32), C.POINTER(_u64)]),
    ("vdf_nova_pow_chain_window", _i, [_vp, C.c_uint, _vp, _sz, C.POINTER(_sz)]),
    ("vdf_nova_forward_body_record", _i, [_i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_forward_tape_eval", _i, [_i, _vp, _vp, _vp, _sz, _u64, _vp, _u64, _sz, _vp, _sz, _u64, _u64, _u64]),
    ("vdf_nova_synthesis_stats", _i, [C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_compress", _i, [_vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_compress_batch", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vdf_nova_verify_compressed", _i, [_vp, _vp, _sz, C.POINTER(_Fe * 3), C.POINTER(_Fe * 3), C.POINTER(_i)]),
    ("vdf_nova_verify_compressed_batch", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_sz), _vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    ("vdf_nova_verify_batch", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_sz), _vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    ("vdf_nova_snark_free", None, [_vp]),
    ("vdf_nova_snark_size", _sz, [_vp]),
    ("vdf_nova_snark_bytes", _i, [_vp, _vp, _sz]),
    ("vdf_nova_snark_set_bytes", _i, [_vp, _vp, _sz]),
    ("vdf_nova_point_compress", _i, [_i, _vp, _vp]),
    ("vdf_nova_point_decompress", _i, [_i, _vp, _vp]),
    ("vdf_nova_snark_serialized_size", _sz, [_vp]),
    ("vdf_nova_snark_serialize", _i, [_vp, _vp, _sz]),
    ("vdf_nova_snark_deserialize", _i, [_vp, _vp, _sz, C.POINTER(_vp)]),
    ("vdf_nova_snark_deserialize_batch", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_i)]),
    ("vdf_nova_verify_wire_batch", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_sz), _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                        C.POINTER(_i)]),
    ("vdf_nova_compress_aggregate", _i, [_vp, _sz, C.POINTER(_vp), C.POINTER(_vp)]),
    ("vdf_nova_verify_aggregate", _i, [_vp, _vp, _sz, C.POINTER(_sz), _vp, _vp, C.POINTER(_i), C.POINTER(C.c_int64)]),
    ("vdf_nova_aggregate_free", None, [_vp]),
    ("vdf_nova_aggregate_count", _sz, [_vp]),
    ("vdf_nova_aggregate_serialized_size", _sz, [_vp]),
    ("vdf_nova_aggregate_serialize", _i, [_vp, _vp, _sz]),
    ("vdf_nova_aggregate_deserialize", _i, [_vp, _vp, _sz, C.POINTER(_vp)]),
    ("vdf_nova_aggregate_fold_instances", _i, [_i, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("vdf_nova_aggregate_fold_instances_device", _i, [_vp, _i, _sz, _vp, _vp, _vp, _vp]),
    ("vdf_nova_verify_aggregate_device", _i, [_vp, _vp, _sz, C.POINTER(_sz), _vp, _vp, C.POINTER(_i), C.POINTER(C.c_int64)]),
    ("vdf_nova_verify_aggregate_wire", _i, [_vp, _vp, _sz, _sz, C.POINTER(_sz), _vp, _vp, C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(_i)]),
    ("vdf_nova_aggregate_verify_times", _i, [C.POINTER(C.c_double)]),
    ("vdf_nova_pp_set_verify_ro_device", _i, [_vp, _i]),
    ("vdf_nova_pp_verify_ro_device", _i, [_vp]),
    ("vdf_nova_pp_verify_ro_stats", _i, [_vp, C.POINTER(_u64)]),
    ("vdf_nova_pp_set_verify_ro_block_device", _i, [_vp, _i]),
    ("vdf_nova_pp_verify_ro_block_device", _i, [_vp]),
    ("vdf_nova_proof_serialized_size", _sz, [_vp]),
    ("vdf_nova_proof_serialize", _i, [_vp, _vp, _sz]),
    ("vdf_nova_proof_deserialize", _i, [_vp, _vp, _sz, C.POINTER(_vp)]),
    # the cycle in either orientation (field = the primary circuit's field, the VDF's)
    ("vdf_nova_public_params_field", _i, [_vp, _i, _u64, _i, _sz, _i, _vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_public_params_custom_field", _i, [_vp, _i, _vp, _i, C.POINTER(_vp)]),
    ("vdf_nova_pp_field", _i, [_vp]),
    ("vdf_nova_eval_and_make_circuits_field", _i, [_i, _i, _u64, _sz, C.POINTER(_State), C.POINTER(_Fe * 3), C.POINTER(_vp)]),
    ("vdf_nova_circuits_from_checkpoints_field", _i, [_i, _u64, _u64, _sz, _vp, C.POINTER(_Fe * 3), C.POINTER(_vp)]),
    ("vdf_nova_circuits_forward_begin_field", _i, [_i, _u64, C.POINTER(_State), C.POINTER(_Fe * 3), C.POINTER(_vp)]),
    ("vdf_nova_circuits_lanes_begin_field", _i, [_i, _u64, _sz, _vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_circuits_field", _i, [_vp]),
    ("vdf_nova_shape_digest_field", _i, [_i, _vp, _u64, _i, _sz, _i, _vp, _vp]),
    ("vdf_nova_shape_export_field", _i, [_i, _u64, _i, _sz, _i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_shape_stencil_field", _i, [_i, _u64, _i, _sz, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_public_params_custom_tuned", _i, [_vp, _i, _vp, _i, _vp, C.POINTER(_vp)]),
    ("vdf_nova_pp_periodic_rows", _i, [_vp] + [C.POINTER(_u64)] * 4),
    ("vdf_nova_shape_export_custom", _i, [_i, _vp, _i, _vp, _vp, _vp, _vp]),
    ("vdf_nova_periodic_rows_detect", _i, [_i, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _u64, _vp, _vp, _vp, _vp] + [C.POINTER(_u64)] * 3),
    ("vdf_nova_periodic_rows_eval", _i, [_i, _vp, _u64, _u64, _sz, _sz, _sz, _sz] + [_vp] * 9),
    ("vdf_nova_shape_periodic_custom", _i, [_i, _vp, _vp, _vp, _vp, _vp] + [C.POINTER(_u64)] * 6),
    ("vdf_nova_aug_synthesize_field", _i, [_i, _vp, _i, _u64, _i, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz), _vp, _vp]),
    # a custom circuit's chain
    ("vdf_nova_custom_chain_from_checkpoints", _i, [_i, _vp, _vp, _u64, _u64, _sz, _vp, _u64, C.POINTER(_vp)]),
    ("vdf_nova_custom_chain_lanes_from_checkpoints", _i, [_i, _vp, _vp, _u64, _u64, _sz, _sz, _vp, _sz, _vp, C.POINTER(_vp)]),
    ("vdf_nova_pp_repeat_lanes", _i, [_vp, C.POINTER(_u64)]),
    ("vdf_nova_custom_chain_from_checkpoints_forward", _i, [_i, _vp, _vp, _u64, _u64, _sz, _vp, _u64, C.POINTER(_vp)]),
    ("vdf_nova_custom_chain_lanes_from_checkpoints_forward", _i, [_i, _vp, _vp, _u64, _u64, _sz, _sz, _vp, _sz, _vp, C.POINTER(_vp)]),
    ("vdf_nova_custom_chain_direction", _i, [_vp]),
    ("vdf_nova_custom_chain_launch_rounds", _i, [_vp, _u64, C.POINTER(_u64)]),
    ("vdf_nova_custom_chain_set_launch_rounds", _i, [_vp, _u64]),
    ("vdf_nova_forward_tape_rebuild_eval_lanes", _i, [_i, _vp, _sz, _vp, _vp, _sz, _u64, _vp, _sz, _u64, _sz, _sz, _vp, _u64, _i, _vp, _vp]),
    ("vdf_nova_custom_chain_materialize", _i, [_vp, _vp, _sz, _sz, _i, _u64, _vp]),
    ("vdf_nova_custom_chain_release", _i, [_vp, _sz, _sz]),
    ("vdf_nova_custom_chain_memory", _i, [_vp, C.POINTER(_sz), C.POINTER(_u64)]),
    ("vdf_nova_custom_chain_host_bytes", _i, [_vp, C.POINTER(_u64)]),
    ("vdf_nova_custom_chain_len", _sz, [_vp]),
    ("vdf_nova_custom_chain_advice", _i, [_vp, _sz, C.POINTER(_vp)]),
    ("vdf_nova_custom_chain_free", None, [_vp]),
    ("vdf_nova_custom_chain_slice", _i, [_u64, _u64, _u64, _u64, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_i)]),
    ("vdf_cs_step_advice", _vp, [_vp]),
    ("vdf_nova_prove_step_custom_chain", _i, [_vp, C.POINTER(_vp), _vp, _vp, _sz, _vp]),
    ("vdf_nova_prove_recursively_custom", _i, [_vp, _vp, _vp, _vp, _sz, C.c_uint32, C.POINTER(_vp)]),
    ("vdf_nova_proof_last_unsat", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("vdf_nova_pp_repeat_rows", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    # a custom chain's lookahead and early rows (tuning custom_ahead)
    ("vdf_cs_is_probe", _i, [_vp]),
    ("vdf_nova_tuning_read", _i, [_vp, _vp]),
    ("vdf_nova_shape_early_rows_custom", _i, [_i, _vp] + [C.POINTER(_u64)] * 4),
    ("vdf_nova_proof_ahead_stats", _i, [_vp] + [C.POINTER(_u64)] * 3),
    # a custom chain that grows, proved while it is evaluated
    ("vdf_nova_custom_chain_begin", _i, [_i, _vp, _i, _vp, _u64, _sz, _vp, _vp, C.POINTER(_vp)]),
    ("vdf_nova_custom_chain_push_checkpoints", _i, [_vp, _u64, _vp, _sz]),
    ("vdf_nova_custom_chain_push_advice", _i, [_vp, _vp, _sz]),
    ("vdf_nova_eval_and_prove_custom", _i, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, C.POINTER(_vp), _vp]),
]:
    if not hasattr(nova_lib, _name):          # AttributeError at call time names the missing entry point
        continue
    getattr(nova_lib, _name).argtypes = _args
    getattr(nova_lib, _name).restype = _res

CIRCUIT_MINROOT_BOUND, CIRCUIT_MINROOT_REFERENCE = 0, 1
CIRCUIT_MINROOT_FORWARD = 3       # the step in the direction of evaluation (include/vdf_nova.h)
STENCIL_FORWARD = 5               # vdf_nova_pp_stencil's code for the forward circuit's stencil
CIRCUIT_MINROOT_FORWARD_LANES = 4 # L forward circuits side by side in one step circuit (public_params_lanes)
STENCIL_FORWARD_LANES = 6         # ... and the code of its stencil
STENCIL_PERIODIC = 7              # a custom circuit's periodic vdf_cs_repeat rows run from their description (tuning periodic_rows)
MAX_LANES = 16
SIDE_PRIMARY, SIDE_SECONDARY = 0, 1
INST_RUNNING_PRIMARY, INST_RUNNING_SECONDARY, INST_FRESH_SECONDARY, INST_FRESH_PRIMARY_LAST = 0, 1, 2, 3
GENS_KNOWN_DLOG, GENS_TRY_AND_INCREMENT, GENS_LABEL_SHAKE = 0, 1, 2
PP_NO_DIGIT_TABLES, PP_NO_EARLY_ROWS = 1, 2
CUSTOM_CHECK_STEPS = 1            # vdf_nova_prove_recursively_custom: scan every step's fresh instance for unsatisfied rows
KERNEL_EVENT_DTYPE = np.dtype([("name", "S24"), ("bytes", "<f8"), ("start_ms", "<f8"), ("end_ms", "<f8")])     # vdf_kernel_event


class NovaTuning(C.Structure):
    """vdf_nova_tuning (include/vdf_nova.h): everything tunable about a parameter set and the prover over it."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("digit_budget_bytes", C.c_uint64)] + [(k, C.c_int32) for k in (
        "digit_window", "early_rows", "stencil", "small_window", "big_window", "packed_commit", "lookahead_early", "gate_accumulate",
        "fold_on_rows", "nifs_ahead", "early_row_parts", "lookahead_priority", "side_accumulate_fill", "verbose", "compress_queues", "rows_at_challenge", "fold_fused",
        "periodic_rows", "custom_ahead")]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class RoParams(C.Structure):
    """vdf_nova_ro_params (include/vdf_nova.h): the random oracle as a parameter block covered by the parameters' digest."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, C.c_int32) for k in (
        "family", "width", "full_rounds", "partial_rounds", "alpha", "challenge_bits", "hash_bits")]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


RO_DEFAULT, RO_NEPTUNE_SHAPED = 0, 1


def ro_preset(which: int = RO_DEFAULT, **fields) -> RoParams:
    """0: this build's default block (Poseidon2-style, width 4); 1: the neptune-shaped block (original Poseidon, width 25,
    8 + 57 rounds; [UPSTREAM-RECALL], unpinned).  Keyword fields replace members (e.g. width=9 for a smaller instance)."""
    r = RoParams()
    _check(nova_lib.vdf_nova_ro_preset(which, C.byref(r)))
    for k, v in fields.items():
        if k not in dict(RoParams._fields_):
            raise KeyError(k)
        setattr(r, k, int(v))
    return r


def _ro_ptr(ro):
    return C.byref(ro) if ro is not None else None


def tuning_default(**fields) -> NovaTuning:
    """The library's defaults (environment overrides applied once per process), with the named fields replaced."""
    t = NovaTuning()
    nova_lib.vdf_nova_tuning_default(C.byref(t))
    for k, v in fields.items():
        if k not in dict(NovaTuning._fields_):
            raise KeyError(k)
        setattr(t, k, int(v))
    return t


def _check(rc: int) -> None:
    if rc != 0:
        raise VdfError(rc, (nova_lib.vdf_nova_last_error() or b"").decode())


def tuning_read(tuning: "NovaTuning | None" = None, struct_size: "int | None" = None) -> NovaTuning:
    """Host only (vdf_nova_tuning_read): the tuning a constructor would run with.  struct_size: hand the struct over as a caller
    compiled against an older header would -- the fields it does not have read as 0."""
    t = NovaTuning()
    if tuning is not None:
        C.memmove(C.byref(t), C.byref(tuning), C.sizeof(NovaTuning))
        if struct_size is not None:
            t.struct_size = struct_size
    out = NovaTuning()
    _check(nova_lib.vdf_nova_tuning_read(C.byref(t) if tuning is not None else None, C.byref(out)))
    return out


def point_compress(aff: np.ndarray, curve: int = 0) -> bytes:
    """32-byte encoding of a point of `curve` given as 8 Montgomery words (x, y); host arithmetic only."""
    a = np.ascontiguousarray(aff, dtype="<u8").reshape(8)
    out = (C.c_uint8 * 32)()
    _check(nova_lib.vdf_nova_point_compress(curve, a.ctypes.data, out))
    return bytes(out)


def point_decompress(data: bytes, curve: int = 0) -> np.ndarray:
    if len(data) != 32:
        raise ValueError("32 bytes")
    out = np.zeros(8, dtype="<u8")
    _check(nova_lib.vdf_nova_point_decompress(curve, (C.c_uint8 * 32).from_buffer_copy(data), out.ctypes.data))
    return out


def ro_constants(field: int) -> np.ndarray:
    """vdf_nova_ro_constants: the default block's 88 round constants of `field` (Montgomery limbs, (88, 4) uint64), in the order
    Context.ro_hash_batch reads them: ext[r][lane] for r = 0..7, then in[0..55]."""
    out = np.zeros((88, 4), dtype="<u8")
    _check(nova_lib.vdf_nova_ro_constants(field, out.ctypes.data))
    return out


def ro_block_constants(field: int, ro: RoParams):
    """vdf_nova_ro_block_constants: a family-1 block's constants of `field` as Context.ro_hash_batch_block reads them -- (rc, mds),
    Montgomery limbs: rc ((full_rounds + partial_rounds) * width, 4) uint64, round-major and lane-minor; mds (width * width, 4),
    row-major.  The default block is refused (ro_constants is its call)."""
    counts = (_sz * 2)()
    _check(nova_lib.vdf_nova_ro_block_constants(_ro_ptr(ro), field, None, None, counts))
    rc, mds = np.zeros((counts[0], 4), dtype="<u8"), np.zeros((counts[1], 4), dtype="<u8")
    _check(nova_lib.vdf_nova_ro_block_constants(_ro_ptr(ro), field, rc.ctypes.data, mds.ctypes.data, counts))
    return rc, mds


def ro_hash_batch_eval(field: int, tag: int, xs, len_: int, n: int, bits: int, out, ro: "RoParams | None" = None) -> None:
    """vdf_nova_ro_hash_batch_eval_ro: the host restatement of Context.ro_hash_batch (ro = None, the default block) and of
    Context.ro_hash_batch_block (another block) -- n messages of len_ elements (message-major Montgomery limbs) hashed into
    out[(n, 4) uint64]; bits = 0: the element, 1..255: the low bits of its canonical integer.  xs and out: numpy arrays or None."""
    ptr = lambda a: None if a is None else a.ctypes.data
    if ro is None:
        _check(nova_lib.vdf_nova_ro_hash_batch_eval(field, tag, ptr(xs), len_, n, bits, ptr(out)))
    else:
        _check(nova_lib.vdf_nova_ro_hash_batch_eval_ro(_ro_ptr(ro), field, tag, ptr(xs), len_, n, bits, ptr(out)))


def ro_hash(field: int, tag: int, xs: np.ndarray, ro: "RoParams | None" = None) -> np.ndarray:
    """The random oracle's sponge (host only): lane 1 after absorbing xs (Montgomery limbs in and out); `ro`: another block."""
    xs = np.ascontiguousarray(xs, dtype="<u8").reshape(-1, 4)
    out = np.zeros(4, dtype="<u8")
    _check(nova_lib.vdf_nova_ro_hash_ro(_ro_ptr(ro), field, tag, xs.ctypes.data, xs.shape[0], out.ctypes.data))
    return out


def shape_digest(t: int, circuit_kind: int = 1, gens_family: int = 1, ro: "RoParams | None" = None):
    """(digest as an integer, sizes[side] = (num_cons, num_vars, nnz)) of the parameters public_params(t) would make."""
    d = (C.c_uint8 * 32)()
    sizes = np.zeros((2, 3), dtype="<u8")
    _check(nova_lib.vdf_nova_shape_digest_ro(_ro_ptr(ro), t, circuit_kind, gens_family, d, sizes.ctypes.data))
    return int.from_bytes(bytes(d), "little"), sizes.tolist()


def shape_stencil(t: int, circuit_kind: int = 1):
    """(variables per round of the MinRoot stencil the early rows match, or 0; first early row; early rows; first round variable)
    -- host only: what public_params(t) would use for the early rows' cross term."""
    b, n, s_ = C.c_uint64(), C.c_uint64(), C.c_uint64()
    per = nova_lib.vdf_nova_shape_stencil(t, circuit_kind, C.byref(b), C.byref(n), C.byref(s_))
    if per < 0:
        _check(-per)
    return per, b.value, n.value, s_.value


def shape_export(t: int, circuit_kind: int = 1, side: int = 0):
    """[(rows uint32[nnz], cols uint32[nnz], vals uint64[nnz, 4])] x 3 (A, B, C) of the shape public_params(t) makes (host only)."""
    nnz = np.zeros(3, dtype="<u8")
    _check(nova_lib.vdf_nova_shape_export(t, circuit_kind, side, nnz.ctypes.data, None, None, None))
    mats = [(np.zeros(int(z), dtype=np.uint32), np.zeros(int(z), dtype=np.uint32), np.zeros((int(z), 4), dtype="<u8")) for z in nnz]
    arr = lambda k: (C.c_void_p * 3)(*[m[k].ctypes.data for m in mats])
    _check(nova_lib.vdf_nova_shape_export(t, circuit_kind, side, nnz.ctypes.data, arr(0), arr(1), arr(2)))
    return mats


# ---- the host-only entry points in either orientation: one general form each (kind FORWARD_LANES with `lanes`; 1 otherwise) ----
def shape_digest_field(field: int, t: int, circuit_kind: int = 1, lanes: int = 1, gens_family: int = 1, ro: "RoParams | None" = None):
    """shape_digest for the orientation `field` (FIELD_FQ: PallasVDF, FIELD_FP: VestaVDF): (digest, sizes[side])."""
    d = (C.c_uint8 * 32)()
    sizes = np.zeros((2, 3), dtype="<u8")
    _check(nova_lib.vdf_nova_shape_digest_field(field, _ro_ptr(ro), t, circuit_kind, lanes, gens_family, d, sizes.ctypes.data))
    return int.from_bytes(bytes(d), "little"), sizes.tolist()


def shape_stencil_field(field: int, t: int, circuit_kind: int = 1, lanes: int = 1):
    """shape_stencil for the orientation `field`: (code 5 / 6 / 4 / 3 or 0; first early row; early rows; first round variable)."""
    b, n, s_ = C.c_uint64(), C.c_uint64(), C.c_uint64()
    code = nova_lib.vdf_nova_shape_stencil_field(field, t, circuit_kind, lanes, C.byref(b), C.byref(n), C.byref(s_))
    if code < 0:
        _check(-code)
    return code, b.value, n.value, s_.value


def shape_export_field(field: int, t: int, circuit_kind: int = 1, lanes: int = 1, side: int = 0):
    """shape_export for the orientation `field`; values in Montgomery form of the side's own scalar field."""
    nnz = np.zeros(3, dtype="<u8")
    _check(nova_lib.vdf_nova_shape_export_field(field, t, circuit_kind, lanes, side, nnz.ctypes.data, None, None, None))
    mats = [(np.zeros(int(z), dtype=np.uint32), np.zeros(int(z), dtype=np.uint32), np.zeros((int(z), 4), dtype="<u8")) for z in nnz]
    arr = lambda k: (C.c_void_p * 3)(*[m[k].ctypes.data for m in mats])
    _check(nova_lib.vdf_nova_shape_export_field(field, t, circuit_kind, lanes, side, nnz.ctypes.data, arr(0), arr(1), arr(2)))
    return mats


def aug_synthesize_field(field: int, side: int, t: int, circuit_kind: int, inputs: "AugInputs", results: Sequence[State] = (),
                         inps: Sequence[State] = (), z0: "Sequence[bytes] | None" = None, zi: "Sequence[bytes] | None" = None,
                         lanes: int = 1, cap: int = 1 << 16, ro=None):
    """One augmented circuit of the orientation `field` synthesised on the host: (W, X, z_next, num_cons).  Side 0: results /
    inps hold one State per lane, z0 / zi (3 * lanes elements) replace those of `inputs` when given."""
    W = np.zeros((cap, 4), dtype="<u8")
    n_out = 3 * lanes if side == 0 else 1
    X, zn = np.zeros((2, 4), dtype="<u8"), np.zeros((max(n_out, 3), 4), dtype="<u8")
    nv, nc = C.c_size_t(), C.c_size_t()
    res = b"".join(s.x + s.y + s.i for s in results) or None
    inp = b"".join(s.x + s.y + s.i for s in inps) or None
    _check(nova_lib.vdf_nova_aug_synthesize_field(field, _ro_ptr(ro), side, t, circuit_kind, lanes, C.addressof(inputs),
                                                  _zn(z0) if z0 is not None else None, _zn(zi) if zi is not None else None, res, inp,
                                                  W.ctypes.data, cap, C.byref(nv), C.byref(nc), X.ctypes.data, zn.ctypes.data))
    return W[:nv.value].copy(), X, zn[:n_out].copy(), nc.value


# ---- the step-circuit seam (include/vdf_nova.h vdf_step_circuit; src/nova/proof.rs:79-153) ---------------------------
_SYNTH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))


class _StepCircuitC(C.Structure):
    _fields_ = [("arity", C.c_size_t), ("synthesize", _SYNTH), ("self", C.c_void_p)]


_BODY = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))


class _RoundBodyC(C.Structure):
    _fields_ = [("n_inv", C.c_size_t), ("n_carry", C.c_size_t), ("n_adv", C.c_size_t), ("body", _BODY), ("self", C.c_void_p)]


class RoundBody:
    """vdf_round_body: one round of a uniform loop.  Subclass (or construct) with n_inv / n_carry / n_adv and
    `body(cs, j, inv, carry, cur, next) -> carry_out` (lists of handles); it runs ONCE, on a recording ConstraintSystem
    (include/vdf_nova.h, vdf_cs_repeat: cur / next are value-only)."""
    n_inv, n_carry, n_adv = 0, 0, 1

    def __init__(self, n_inv=None, n_carry=None, n_adv=None, body=None):
        for k, v in (("n_inv", n_inv), ("n_carry", n_carry), ("n_adv", n_adv), ("body", body)):
            if v is not None:
                setattr(self, k, v)

    def body(self, cs, j, inv, carry, cur, next):
        raise NotImplementedError

    def _c(self):
        def cb(_self, cs, j, inv, carry, cur, nxt, out):
            try:
                res = self.body(ConstraintSystem(cs), j, [inv[k] for k in range(self.n_inv)], [carry[k] for k in range(self.n_carry)],
                                [cur[k] for k in range(self.n_adv)], [nxt[k] for k in range(self.n_adv)])
                res = list(res or [])
                if len(res) != self.n_carry:
                    raise ValueError("a round body returns n_carry handles")
                for k in range(self.n_carry):
                    out[k] = res[k]
                return 0
            except Exception as e:            # must not unwind through the C frames
                self._error = e
                return 1
        self._error = None
        self._cb = _BODY(cb)                  # kept alive with the body
        self._struct = _RoundBodyC(self.n_inv, self.n_carry, self.n_adv, self._cb, None)
        return self._struct


_RECORDINGS = []      # one dict per record_*_body call in progress: address -> the numpy table its body handed to ConstraintSystem.tab


def _record(call, field: int, body, tape: RoundTape) -> RoundTape:
    """One recording: the tables the body names are remembered for this call only (whether it returns or raises), and the tape
    that comes back names its table by address -- it keeps that array alive from then on."""
    seen = {}
    _RECORDINGS.append(seen)
    try:
        rc = call(field, C.addressof(body._c()), C.addressof(tape.ops), tape.consts.ctypes.data, C.addressof(tape.c))
    finally:
        _RECORDINGS.pop()
    _reraise(body)
    _check(rc)
    if tape.c.tab_rows:
        tape.table = seen[tape.c.table]
    return tape


def record_round_body(body: RoundBody, field: int = FIELD_FQ) -> RoundTape:
    """Host only: the body recorded and compiled into the tape Context.round_tape_run / round_tape_eval take."""
    return _record(nova_lib.vdf_nova_round_body_record, field, body, RoundTape())


def round_tape_eval(field: int, tape: RoundTape, t: int, inv, advice) -> np.ndarray:
    """Host only: what Context.round_tape_run writes, uint64[t * n_vars, 4]; inv, advice: uint64[., 4] arrays (Montgomery form)."""
    inv = np.ascontiguousarray(inv, dtype="<u8").reshape(-1, 4)
    advice = np.ascontiguousarray(advice, dtype="<u8").reshape(-1, 4)
    if inv.shape[0] < tape.c.n_inv or advice.shape[0] < (t + 1) * tape.c.n_adv:
        raise ValueError("inv or advice shorter than the tape reads")
    out = np.zeros((t * tape.c.n_vars, 4), dtype="<u8")
    _check(nova_lib.vdf_nova_round_tape_eval(field, C.addressof(tape.c), t, inv.ctypes.data if tape.c.n_inv else None, advice.ctypes.data,
                                             out.ctypes.data))
    return out


def round_tape_eval_lanes(field: int, tape: RoundTape, t: int, lanes: int, inv, advice, lane_stride: int) -> np.ndarray:
    """Host only: what Context.round_tape_run_lanes writes, uint64[lanes * t * n_vars, 4]; inv: lanes * n_inv elements, advice:
    lane l's t + 1 entries from entry l * lane_stride on."""
    inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
    advice = np.ascontiguousarray(advice, dtype="<u8").reshape(-1, 4)
    ok_shape = 0 < lanes <= 16 and lane_stride >= t + 1
    if ok_shape and (inv.shape[0] < lanes * tape.c.n_inv or advice.shape[0] < ((lanes - 1) * lane_stride + t + 1) * tape.c.n_adv):
        raise ValueError("inv or advice shorter than the tape reads")
    out = np.zeros((max(lanes, 0) * t * tape.c.n_vars, 4), dtype="<u8")
    _check(nova_lib.vdf_nova_round_tape_eval_lanes(field, C.addressof(tape.c), t, lanes, inv.ctypes.data if tape.c.n_inv else None,
                                                   advice.ctypes.data, lane_stride, out.ctypes.data))
    return out


_WALK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))


class _WalkBodyC(C.Structure):
    _fields_ = [("n_inv", C.c_size_t), ("n_adv", C.c_size_t), ("body", _WALK), ("self", C.c_void_p)]


class WalkBody:
    """vdf_walk_body: the fast direction of a round, advice entry j computed from entry j + 1.  Subclass (or construct) with
    n_inv / n_adv and `body(cs, j, inv, next) -> cur` (n_adv handles); it runs ONCE, on a recording ConstraintSystem where add,
    sub, scale, const and mul are value arithmetic and nothing else is allowed (include/vdf_nova.h)."""
    n_inv, n_adv = 0, 1

    def __init__(self, n_inv=None, n_adv=None, body=None):
        for k, v in (("n_inv", n_inv), ("n_adv", n_adv), ("body", body)):
            if v is not None:
                setattr(self, k, v)

    def body(self, cs, j, inv, next):
        raise NotImplementedError

    def _c(self):
        def cb(_self, cs, j, inv, nxt, out):
            try:
                res = list(self.body(ConstraintSystem(cs), j, [inv[k] for k in range(self.n_inv)], [nxt[k] for k in range(self.n_adv)]) or [])
                if len(res) != self.n_adv:
                    raise ValueError("a walk body returns n_adv handles")
                for k in range(self.n_adv):
                    out[k] = res[k]
                return 0
            except Exception as e:            # must not unwind through the C frames
                self._error = e
                return 1
        self._error = None
        self._cb = _WALK(cb)                  # kept alive with the body
        self._struct = _WalkBodyC(self.n_inv, self.n_adv, self._cb, None)
        return self._struct


def record_walk_body(body: WalkBody, field: int = FIELD_FQ) -> RoundTape:
    """Host only: the walk body recorded and compiled into the walk tape Context.round_tape_walk / walk_tape_eval take."""
    return _record(nova_lib.vdf_nova_walk_body_record, field, body, RoundTape())


def walk_tape_eval(field: int, tape: RoundTape, inv, entries: np.ndarray, n: int, rounds: int, trace: "np.ndarray | None" = None,
                   walk_stride: int = 0, top: int = 0, group: int = 0, group_stride: int = 0, j_base: int = 0, j_group_step: int = 0,
                   heads: bool = False, expect: "np.ndarray | None" = None, ok: "np.ndarray | None" = None) -> None:
    """Host only: Context.round_tape_walk on the host, in place over numpy arrays (entries / trace / expect uint64[., 4]
    Montgomery, ok int32[n]); the same arguments and the same refusals.  The arrays are checked against what the walks touch."""
    def arr(x, dtype, what):
        if x is None:
            return None
        if not isinstance(x, np.ndarray) or x.dtype != np.dtype(dtype) or not x.flags["C_CONTIGUOUS"] or not x.flags["WRITEABLE"]:
            raise ValueError("%s: a writable C-contiguous %s array" % (what, dtype))
        return x
    na = tape.c.n_adv
    inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
    entries, trace, expect, ok = arr(entries, "<u8", "entries"), arr(trace, "<u8", "trace"), arr(expect, "<u8", "expect"), arr(ok, "<i4", "ok")
    if inv.shape[0] < tape.c.n_inv or entries.size < 4 * n * na or (expect is not None and expect.size < 4 * n * na) or \
            (ok is not None and ok.size < n):
        raise ValueError("inv, entries, expect or ok shorter than the walks read")
    if trace is not None and n and rounds and top + 1 >= rounds:
        g = group or n
        last = ((n - 1) // g) * (group_stride if group else 0) + (min(n, g) - 1) * walk_stride + top
        if trace.size < 4 * (last + 1) * na:
            raise ValueError("trace shorter than the walks write")
    _check(nova_lib.vdf_nova_walk_tape_eval(field, C.addressof(tape.c), inv.ctypes.data if tape.c.n_inv else None, entries.ctypes.data, n, rounds,
                                            trace.ctypes.data if trace is not None else None, walk_stride, top, group, group_stride, j_base,
                                            j_group_step, int(bool(heads)), expect.ctypes.data if expect is not None else None,
                                            ok.ctypes.data if ok is not None else None))


def walk_tape_eval_lanes(field: int, tape: RoundTape, lanes: int, inv, entries: np.ndarray, n: int, rounds: int,
                         trace: "np.ndarray | None" = None, walk_stride: int = 0, top: int = 0, group: int = 0, group_stride: int = 0,
                         j_base=None, j_group_step: int = 0, heads: bool = False, expect: "np.ndarray | None" = None,
                         ok: "np.ndarray | None" = None) -> None:
    """Host only: Context.round_tape_walk_lanes on the host, in place over numpy arrays as walk_tape_eval; inv: lanes * n_inv
    elements, j_base: `lanes` ints (default zeros).  The same arguments and the same refusals."""
    def arr(x, dtype, what):
        if x is None:
            return None
        if not isinstance(x, np.ndarray) or x.dtype != np.dtype(dtype) or not x.flags["C_CONTIGUOUS"] or not x.flags["WRITEABLE"]:
            raise ValueError("%s: a writable C-contiguous %s array" % (what, dtype))
        return x
    na = tape.c.n_adv
    inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
    jb = np.ascontiguousarray([0] * max(lanes, 1) if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
    entries, trace, expect, ok = arr(entries, "<u8", "entries"), arr(trace, "<u8", "trace"), arr(expect, "<u8", "expect"), arr(ok, "<i4", "ok")
    if 0 < lanes <= 16:
        if inv.shape[0] < lanes * tape.c.n_inv or jb.size < lanes or entries.size < 4 * n * na or \
                (expect is not None and expect.size < 4 * n * na) or (ok is not None and ok.size < n):
            raise ValueError("inv, j_base, entries, expect or ok shorter than the walks read")
    if trace is not None and n and rounds and top + 1 >= rounds:
        g = group or n
        last = ((n - 1) // g) * (group_stride if group else 0) + (min(n, g) - 1) * walk_stride + top
        if trace.size < 4 * (last + 1) * na:
            raise ValueError("trace shorter than the walks write")
    _check(nova_lib.vdf_nova_walk_tape_eval_lanes(field, C.addressof(tape.c), lanes, inv.ctypes.data if tape.c.n_inv else None,
                                                  entries.ctypes.data, n, rounds, trace.ctypes.data if trace is not None else None,
                                                  walk_stride, top, group, group_stride, jb.ctypes.data, j_group_step, int(bool(heads)),
                                                  expect.ctypes.data if expect is not None else None,
                                                  ok.ctypes.data if ok is not None else None))


def record_forward_body(body: WalkBody, field: int = FIELD_FQ) -> RoundTape:
    """Host only: a WalkBody whose `next` argument is the entry stood on (entry j) and whose result is entry j + 1 -- the slow
    direction, with ConstraintSystem.pow -- recorded into the forward walk tape Context.round_tape_forward_walk /
    round_tape_eval_batch / forward_tape_eval take."""
    return _record(nova_lib.vdf_nova_forward_body_record, field, body, RoundTape())


def forward_tape_eval(field: int, tape: RoundTape, inv, entries: np.ndarray, n: int, rounds: int, checkpoints: "np.ndarray | None" = None,
                      every: int = 0, cp_stride: int = 0, trace: "np.ndarray | None" = None, walk_stride: int = 0, base: int = 0,
                      j_base: int = 0, j_walk_step: int = 0) -> None:
    """Host only: Context.round_tape_forward_walk on the host, in place over numpy arrays (entries / checkpoints / trace
    uint64[., 4] Montgomery); the same arguments and the same refusals.  The arrays are checked against what the walks touch."""
    def arr(x, what):
        if x is None:
            return None
        if not isinstance(x, np.ndarray) or x.dtype != np.dtype("<u8") or not x.flags["C_CONTIGUOUS"] or not x.flags["WRITEABLE"]:
            raise ValueError("%s: a writable C-contiguous <u8 array" % what)
        return x
    na = tape.c.n_adv
    inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
    entries, checkpoints, trace = arr(entries, "entries"), arr(checkpoints, "checkpoints"), arr(trace, "trace")
    if inv.shape[0] < tape.c.n_inv or entries.size < 4 * n * na:
        raise ValueError("inv or entries shorter than the walks read")
    if n and rounds:
        if trace is not None and trace.size < 4 * ((n - 1) * walk_stride + base + rounds + 1) * na:
            raise ValueError("trace shorter than the walks write")
        if checkpoints is not None and every and checkpoints.size < 4 * ((n - 1) * cp_stride + (base + rounds) // every + 1) * na:
            raise ValueError("checkpoints shorter than the walks write")
    _check(nova_lib.vdf_nova_forward_tape_eval(field, C.addressof(tape.c), inv.ctypes.data if tape.c.n_inv else None, entries.ctypes.data, n, rounds,
                                               checkpoints.ctypes.data if checkpoints is not None else None, every, cp_stride,
                                               trace.ctypes.data if trace is not None else None, walk_stride, base, j_base, j_walk_step))


def forward_tape_rebuild_eval_lanes(field: int, forward_tape: RoundTape, lanes: int, inv, entries: np.ndarray, n: int, rounds: int,
                                    trace: "np.ndarray | None" = None, walk_stride: int = 0, base: int = 0, group: int = 0,
                                    group_stride: int = 0, j_base=None, j_group_step: int = 0, heads: bool = False,
                                    expect: "np.ndarray | None" = None, ok: "np.ndarray | None" = None) -> None:
    """Host only: Context.round_tape_rebuild_lanes on the host, in place over numpy arrays as walk_tape_eval_lanes; inv: lanes *
    n_inv elements, j_base: `lanes` ints (default zeros).  The same arguments and the same refusals; the arrays are checked against
    what the walks touch."""
    def arr(x, dtype, what):
        if x is None:
            return None
        if not isinstance(x, np.ndarray) or x.dtype != np.dtype(dtype) or not x.flags["C_CONTIGUOUS"] or not x.flags["WRITEABLE"]:
            raise ValueError("%s: a writable C-contiguous %s array" % (what, dtype))
        return x
    na = forward_tape.c.n_adv
    inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
    jb = None if j_base is False else np.ascontiguousarray([0] * max(lanes, 1) if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
    entries, trace, expect, ok = arr(entries, "<u8", "entries"), arr(trace, "<u8", "trace"), arr(expect, "<u8", "expect"), arr(ok, "<i4", "ok")
    if 0 < lanes <= 16:
        if inv.shape[0] < lanes * forward_tape.c.n_inv or (jb is not None and jb.size < lanes) or (entries is not None and entries.size < 4 * n * na) or \
                (expect is not None and expect.size < 4 * n * na) or (ok is not None and ok.size < n):
            raise ValueError("inv, j_base, entries, expect or ok shorter than the walks read")
    if trace is not None and n and rounds:
        g = group or n
        last = ((n - 1) // g) * (group_stride if group else 0) + (min(n, g) - 1) * walk_stride + base + rounds
        if trace.size < 4 * (last + 1) * na:
            raise ValueError("trace shorter than the walks write")
    _check(nova_lib.vdf_nova_forward_tape_rebuild_eval_lanes(field, C.addressof(forward_tape.c), lanes, inv.ctypes.data if forward_tape.c.n_inv else None,
                                                             entries.ctypes.data if entries is not None else None, n, rounds,
                                                             trace.ctypes.data if trace is not None else None, walk_stride, base, group,
                                                             group_stride, jb.ctypes.data if jb is not None else None, j_group_step,
                                                             int(bool(heads)), expect.ctypes.data if expect is not None else None,
                                                             ok.ctypes.data if ok is not None else None))


POW_ACC, POW_NONE, POW_CHAIN_MAX_STEPS, POW_CHAIN_MAX_TMP = 0xFE, 0xFF, 95, 12      # VDF_POW_*


def _pow_steps(steps):
    """[(src, squarings, mul, dst)] -> a ctypes array of vdf_pow_step (one spare element, so that no chain is a null pointer)"""
    arr = (C.c_uint8 * (4 * (len(steps) + 1)))()
    for k, st in enumerate(steps):
        if len(st) != 4 or any(not 0 <= int(v) <= 255 for v in st):
            raise ValueError("a step is (src, squarings, mul, dst), each a byte")
        arr[4 * k:4 * k + 4] = [int(v) for v in st]
    return arr


def pow_chain_exponent(steps):
    """Host only (vdf_nova_pow_chain_exponent): validates the chain and returns (E, n_tmp, products); VdfError(BAD_ARG) names the
    step of an invalid one."""
    e, n_tmp, products = (C.c_uint64 * 4)(), C.c_uint32(), C.c_uint64()
    _check(nova_lib.vdf_nova_pow_chain_exponent(_pow_steps(steps), len(steps), e, C.byref(n_tmp), C.byref(products)))
    return sum(int(e[k]) << (64 * k) for k in range(4)), n_tmp.value, products.value


def pow_chain_window(e: int, window: int = 4, cap: int = POW_CHAIN_MAX_STEPS):
    """Host only (vdf_nova_pow_chain_window): a left-to-right sliding-window chain for any exponent 1 <= e < 2^256, as a list of
    (src, squarings, mul, dst); window 2 .. 4."""
    if not 0 <= e < 1 << 256:
        raise ValueError("the exponent is an integer in [0, 2^256)")
    arr, n = (C.c_uint8 * (4 * (cap + 1)))(), C.c_size_t()
    _check(nova_lib.vdf_nova_pow_chain_window((C.c_uint64 * 4)(*[(e >> (64 * k)) & (2**64 - 1) for k in range(4)]), window, arr, cap, C.byref(n)))
    return [tuple(arr[4 * k:4 * k + 4]) for k in range(n.value)]


class ConstraintSystem:
    """The vdf_cs a step circuit's synthesize receives: numbers are opaque handles; field elements cross as 32-byte
    Montgomery limbs of the primary circuit's field (Fq, or Fp under public_params_custom(..., field=FIELD_FP))."""

    def __init__(self, handle):
        self.h = handle

    @property
    def is_witness(self) -> bool:
        return bool(nova_lib.vdf_cs_is_witness(self.h))

    @property
    def is_probe(self) -> bool:
        """vdf_cs_is_probe: this witness synthesis is the extra one of tuning custom_ahead -- its values are kept by nobody, and
        its `repeat` only records the body and the values of inv (include/vdf_nova.h, THE PROBE)."""
        return bool(nova_lib.vdf_cs_is_probe(self.h))

    def const(self, k: bytes) -> int:
        return nova_lib.vdf_cs_const(self.h, C.byref(_Fe.from_buffer_copy(k)))

    def add(self, a: int, b: int) -> int:
        return nova_lib.vdf_cs_add(self.h, a, b)

    def sub(self, a: int, b: int) -> int:
        return nova_lib.vdf_cs_sub(self.h, a, b)

    def scale(self, a: int, k: bytes) -> int:
        return nova_lib.vdf_cs_scale(self.h, a, C.byref(_Fe.from_buffer_copy(k)))

    def alloc(self, value: bytes = None) -> int:
        return nova_lib.vdf_cs_alloc(self.h, C.byref(_Fe.from_buffer_copy(value)) if value is not None else None)

    def mul(self, a: int, b: int) -> int:
        return nova_lib.vdf_cs_mul(self.h, a, b)

    def pow(self, a: int, e: int) -> int:
        """a ^ e, e a plain integer below 2^256: value arithmetic of a forward body (record_forward_body) only; anywhere else
        the failure flag."""
        if not 0 <= e < 1 << 256:
            raise ValueError("the exponent is an integer in [0, 2^256)")
        return nova_lib.vdf_cs_pow(self.h, a, (C.c_uint64 * 4)(*[(e >> (64 * k)) & (2**64 - 1) for k in range(4)]))

    def tab(self, table: np.ndarray, col: int) -> int:
        """The round constant of round j from a table: table[j mod rows][col], table a C-contiguous uint64[rows, cols, 4] array in
        Montgomery form that the caller keeps alive and hands over UNCHANGED in every call -- a body has one table, named by its
        address (include/vdf_nova.h vdf_cs_tab).  Legal only while a round, walk or forward body is recorded."""
        if not (isinstance(table, np.ndarray) and table.dtype == np.dtype("<u8") and table.ndim == 3 and table.shape[2] == 4 and
                table.flags["C_CONTIGUOUS"]):
            raise ValueError("a table is a C-contiguous uint64[rows, cols, 4] array")
        if _RECORDINGS:                        # (outside record_*_body nothing is kept: the caller keeps the table alive)
            _RECORDINGS[-1][table.ctypes.data] = table
        return nova_lib.vdf_cs_tab(self.h, table.ctypes.data, table.shape[0], table.shape[1], col)

    def pow_chain(self, a: int, steps) -> int:
        """a ^ E by the caller's addition chain: steps = [(src, squarings, mul, dst)] (include/vdf_hip.h vdf_pow_step; POW_ACC /
        POW_NONE), E its exponent (pow_chain_exponent).  Value arithmetic of a forward body only, as `pow`; anywhere else, and for
        an invalid chain, the failure flag."""
        arr = _pow_steps(steps)
        return nova_lib.vdf_cs_pow_chain(self.h, a, arr, len(steps))

    def enforce(self, a: int, b: int, c: int) -> None:
        _check(nova_lib.vdf_cs_enforce(self.h, a, b, c))

    def value(self, a: int) -> bytes:
        out = _Fe()
        _check(nova_lib.vdf_cs_value(self.h, a, C.byref(out)))
        return bytes(out)

    def alloc_from(self, src: int) -> int:
        """A new variable with src's value and no constraint."""
        return nova_lib.vdf_cs_alloc_from(self.h, src)

    def step_advice(self) -> Optional[int]:
        """vdf_cs_step_advice: the device address of the step's trace inside a synthesize driven by prove_step_custom_chain /
        prove_recursively_custom, in witness mode; None in every other case.  What `repeat` takes as advice."""
        return nova_lib.vdf_cs_step_advice(self.h)

    def repeat(self, body: "RoundBody", t: int, inv, carry_in, advice=None):
        """vdf_cs_repeat: t repetitions of `body`; returns the carry_out handles.  advice: (t + 1) x n_adv elements, entry-major --
        bytes or a uint64[., 4] array (host), a device tensor or an address (device: the rounds then run on the GPU); None while
        the shape is recorded."""
        if len(inv) != body.n_inv or len(carry_in) != body.n_carry:
            raise ValueError("inv / carry_in do not match the body's n_inv / n_carry")
        if isinstance(advice, (bytes, bytearray)):
            advice = np.frombuffer(bytes(advice), dtype="<u8")
        if isinstance(advice, np.ndarray):
            advice = np.ascontiguousarray(advice, dtype="<u8")
            if advice.size * 8 < (t + 1) * body.n_adv * 32:
                raise ValueError("advice is shorter than (t + 1) * n_adv elements")
        if hasattr(advice, "data_ptr") and advice.numel() * advice.element_size() < (t + 1) * body.n_adv * 32:
            raise ValueError("advice is shorter than (t + 1) * n_adv elements")
        U = C.c_uint32
        cin, cout, invs = (U * max(1, body.n_carry))(*carry_in), (U * max(1, body.n_carry))(), (U * max(1, body.n_inv))(*inv)
        rc = nova_lib.vdf_cs_repeat(self.h, C.addressof(body._c()), t, invs, cin, _ptr(advice), cout)
        _reraise(body)
        _check(rc)
        return [cout[k] for k in range(body.n_carry)]

    def repeat_lanes(self, body: "RoundBody", t: int, lanes: int, inv, carry_in, advice=None, lane_stride: Optional[int] = None):
        """vdf_cs_repeat_lanes: `lanes` chains through one recorded body, lane after lane; inv / carry_in: lanes * n_inv / lanes *
        n_carry handles, lane-major; returns the lanes * n_carry carry_out handles.  advice as in `repeat`, lane l's t + 1 entries
        from entry l * lane_stride on (default t + 1)."""
        lane_stride = t + 1 if lane_stride is None else lane_stride
        if len(inv) != lanes * body.n_inv or len(carry_in) != lanes * body.n_carry:
            raise ValueError("inv / carry_in do not match lanes * n_inv / lanes * n_carry")
        need = ((lanes - 1) * lane_stride + t + 1) * body.n_adv * 32 if lanes > 0 and lane_stride >= t + 1 else 0
        if isinstance(advice, (bytes, bytearray)):
            advice = np.frombuffer(bytes(advice), dtype="<u8")
        if isinstance(advice, np.ndarray):
            advice = np.ascontiguousarray(advice, dtype="<u8")
            if advice.size * 8 < need:
                raise ValueError("advice is shorter than the lanes read")
        if hasattr(advice, "data_ptr") and advice.numel() * advice.element_size() < need:
            raise ValueError("advice is shorter than the lanes read")
        U = C.c_uint32
        n_c, n_i = max(1, len(carry_in)), max(1, len(inv))
        cin, cout, invs = (U * n_c)(*carry_in), (U * n_c)(), (U * n_i)(*inv)
        rc = nova_lib.vdf_cs_repeat_lanes(self.h, C.addressof(body._c()), t, lanes, invs, cin, _ptr(advice), lane_stride, cout)
        _reraise(body)
        _check(rc)
        return [cout[k] for k in range(len(carry_in))]


class StepCircuit:
    """trait StepCircuit (src/nova/proof.rs:79-153) for a circuit written by the host: subclass with `arity` and
    `synthesize(cs, z_in) -> z_out` (lists of handles).  The instance is handed to the library as a vdf_step_circuit."""
    arity = 1

    def synthesize(self, cs: ConstraintSystem, z_in):
        raise NotImplementedError

    def _c(self):
        def cb(_self, cs, zin, zout):
            try:
                out = self.synthesize(ConstraintSystem(cs), [zin[k] for k in range(self.arity)])
                for k in range(self.arity):
                    zout[k] = out[k]
                return 0
            except Exception as e:            # must not unwind through the C frames
                self._error = e
                return 1
        self._cb = _SYNTH(cb)                 # kept alive with the circuit
        self._struct = _StepCircuitC(self.arity, self._cb, None)
        return self._struct


def shape_digest_custom(circuit: StepCircuit, gens_family: int = 1):
    """Host only: (digest, sizes) of the parameters public_params_custom would make for this circuit."""
    d = (C.c_uint8 * 32)()
    sizes = np.zeros((2, 3), dtype="<u8")
    rc = nova_lib.vdf_nova_shape_digest_custom(C.byref(circuit._c()), gens_family, d, sizes.ctypes.data)
    _reraise(circuit)
    _check(rc)
    return int.from_bytes(bytes(d), "little"), sizes.tolist()


def _reraise(circuit) -> None:
    e = getattr(circuit, "_error", None)
    if e is not None:
        circuit._error = None
        raise e


def shape_export_custom(circuit: StepCircuit, field: int = FIELD_FQ, side: int = 0):
    """shape_export for a custom primary circuit synthesised over `field` (host only)."""
    nnz = np.zeros(3, dtype="<u8")
    cc = circuit._c()
    rc = nova_lib.vdf_nova_shape_export_custom(field, C.byref(cc), side, nnz.ctypes.data, None, None, None)
    _reraise(circuit)
    _check(rc)
    mats = [(np.zeros(int(z), dtype=np.uint32), np.zeros(int(z), dtype=np.uint32), np.zeros((int(z), 4), dtype="<u8")) for z in nnz]
    arr = lambda k: (C.c_void_p * 3)(*[m[k].ctypes.data for m in mats])
    rc = nova_lib.vdf_nova_shape_export_custom(field, C.byref(cc), side, nnz.ctypes.data, arr(0), arr(1), arr(2))
    _reraise(circuit)
    _check(rc)
    return mats


def periodic_rows_detect(field: int, mats, seg_begin: int, n_vars: int, row_begin: int, n_cons: int, t: int) -> "PeriodicRows | None":
    """Host only.  Are the rows row_begin + j * n_cons + c of the COO triples `mats` (as shape_export gives them) periodic from
    some lead in 0 .. 4 on?  The description (its lead, row_begin, row_count set), or None.  Every triple of every periodic
    repetition is compared with the pattern."""
    mats = [(np.ascontiguousarray(r, dtype=np.uint32), np.ascontiguousarray(c, dtype=np.uint32), np.ascontiguousarray(v, dtype="<u8"))
            for r, c, v in mats]
    nnz = np.array([m[0].shape[0] for m in mats], dtype="<u8")
    arr = lambda k: (C.c_void_p * 3)(*[m[k].ctypes.data for m in mats])
    pr = PeriodicRows()
    lead, first, count = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = nova_lib.vdf_nova_periodic_rows_detect(field, nnz.ctypes.data, arr(0), arr(1), arr(2), seg_begin, n_vars, row_begin, n_cons, t,
                                                pr.row_start.ctypes.data, C.addressof(pr.terms), pr.consts.ctypes.data, C.addressof(pr.c),
                                                C.byref(lead), C.byref(first), C.byref(count))
    if rc < 0:
        _check(-rc)
    if rc == 0:
        return None
    pr.lead, pr.row_begin, pr.row_count = lead.value, first.value, count.value
    return pr


def shape_periodic_custom(circuit: StepCircuit, field: int = FIELD_FQ):
    """Host only: the detection public_params_custom makes.  (description or None, info) with info = dict(seg_begin, num_cons,
    num_cols) of the primary shape."""
    pr = PeriodicRows()
    v = [C.c_uint64() for _ in range(6)]
    rc = nova_lib.vdf_nova_shape_periodic_custom(field, C.byref(circuit._c()), pr.row_start.ctypes.data, C.addressof(pr.terms),
                                                 pr.consts.ctypes.data, C.addressof(pr.c), *[C.byref(x) for x in v])
    _reraise(circuit)
    if rc < 0:
        _check(-rc)
    info = dict(seg_begin=v[0].value, num_cons=v[4].value, num_cols=v[5].value)
    if rc == 0:
        return None, info
    pr.lead, pr.row_begin, pr.row_count = v[1].value, v[2].value, v[3].value
    return pr, info


def shape_early_rows_custom(circuit: StepCircuit, field: int = FIELD_FQ) -> dict:
    """Host only: the early rows public_params_custom(..., custom_ahead=2) would find -- dict(row_begin, rows, zin_begin,
    seg_begin); rows = 0 for a run shorter than 64 rows or a circuit without a repeat."""
    v = [C.c_uint64() for _ in range(4)]
    rc = nova_lib.vdf_nova_shape_early_rows_custom(field, C.byref(circuit._c()), *[C.byref(x) for x in v])
    _reraise(circuit)
    _check(rc)
    return dict(row_begin=v[0].value, rows=v[1].value, zin_begin=v[2].value, seg_begin=v[3].value)


def periodic_rows_eval(field: int, rows: "PeriodicRows", j_first: int, reps: int, seg_begin: int, row_begin: int, num_cols: int,
                       num_cons: int, z2, az1, bz1, cz1, u1, az2, bz2, cz2, T) -> None:
    """Host only: Context.nifs_cross_term_periodic restated over numpy arrays (uint64[n, 4], written in place), byte for byte."""
    for a in (z2, az1, bz1, cz1, u1, az2, bz2, cz2, T):
        if not (isinstance(a, np.ndarray) and a.dtype == np.dtype("<u8") and a.flags["C_CONTIGUOUS"]):
            raise TypeError("periodic_rows_eval takes C-contiguous uint64 arrays")
    _check(nova_lib.vdf_nova_periodic_rows_eval(field, C.addressof(rows.c), j_first, reps, seg_begin, row_begin, num_cols, num_cons,
                                                *[a.ctypes.data for a in (z2, az1, bz1, cz1, u1, az2, bz2, cz2, T)]))


def public_params_custom(ctx: Context, circuit: StepCircuit, gens_family: int = GENS_TRY_AND_INCREMENT,
                         field: int = FIELD_FQ, tuning: "NovaTuning | None" = None, **tune) -> "NovaVDFPublicParams":
    """`field`: the orientation -- the field the circuit is synthesised over (FIELD_FP: G1 = Vesta).  `tuning` / keyword fields of
    vdf_nova_tuning (e.g. periodic_rows=1, custom_ahead=2): vdf_nova_public_params_custom_tuned."""
    h = C.c_void_p()
    if tuning is not None or tune:
        t = tuning if tuning is not None else tuning_default()
        for k, v in tune.items():
            if k not in dict(NovaTuning._fields_):
                raise KeyError(k)
            setattr(t, k, int(v))
        rc = nova_lib.vdf_nova_public_params_custom_tuned(ctx.handle, field, C.byref(circuit._c()), gens_family, C.byref(t), C.byref(h))
    elif field == FIELD_FQ:
        rc = nova_lib.vdf_nova_public_params_custom(ctx.handle, C.byref(circuit._c()), gens_family, C.byref(h))
    else:
        rc = nova_lib.vdf_nova_public_params_custom_field(ctx.handle, field, C.byref(circuit._c()), gens_family, C.byref(h))
    _reraise(circuit)
    _check(rc)
    pp = NovaVDFPublicParams(ctx, h.value, 0)
    pp.arity = circuit.arity
    return pp


def _zn(vals: Sequence[bytes]):
    return (_Fe * len(vals))(*[_Fe.from_buffer_copy(v) for v in vals])


def synthesis_stats() -> Tuple[int, int]:
    """(slope inverses queued by the batched pre-pass, queue misses) of this thread's last augmented-circuit synthesis."""
    q, m = C.c_uint64(), C.c_uint64()
    _check(nova_lib.vdf_nova_synthesis_stats(C.byref(q), C.byref(m)))
    return q.value, m.value


class AugInputs(C.Structure):     # vdf_nova_aug_inputs
    _fields_ = [("params", _Fe), ("i", _Fe), ("z0", _Fe * 3), ("zi", _Fe * 3),
                ("U_comm_W", _Fe * 2), ("U_comm_E", _Fe * 2), ("U_u", _Fe), ("U_X", _Fe * 2),
                ("u_comm_W", _Fe * 2), ("u_X", _Fe * 2), ("T", _Fe * 2)]


def aug_synthesize(side: int, t: int, circuit_kind: int, inputs: AugInputs, result=None, inp=None, cap: int = 1 << 16, ro=None):
    """One augmented circuit synthesised on the host: (W, X, z_next, num_cons)."""
    W = np.zeros((cap, 4), dtype="<u8")
    X, zn = np.zeros((2, 4), dtype="<u8"), np.zeros((3, 4), dtype="<u8")
    nv, nc = C.c_size_t(), C.c_size_t()
    r = C.byref(result._c()) if result is not None else None
    i = C.byref(inp._c()) if inp is not None else None
    _check(nova_lib.vdf_nova_aug_synthesize_ro(_ro_ptr(ro), side, t, circuit_kind, C.addressof(inputs), C.cast(r, _vp) if r else None,
                                               C.cast(i, _vp) if i else None, W.ctypes.data, cap, C.byref(nv), C.byref(nc),
                                               X.ctypes.data, zn.ctypes.data))
    return W[:nv.value].copy(), X, zn[:3 if side == 0 else 1].copy(), nc.value


def _z(vals: Sequence[bytes]):
    return (_Fe * len(vals))(*[_Fe.from_buffer_copy(v) for v in vals])


class NovaVDFPublicParams:        # src/nova/proof.rs:38-43
    def __init__(self, ctx: Context, handle: int, t: int):
        self.ctx, self.handle, self.num_iters_per_step = ctx, handle, t
        self._proofs = weakref.WeakSet()         # proofs made under these parameters: freed before them
        ctx._children.add(self)

    def sizes(self, side: int = 0) -> dict:
        v = [C.c_uint64() for _ in range(5)]
        _check(nova_lib.vdf_nova_pp_sizes(self.handle, side, *[C.byref(x) for x in v]))
        return dict(zip(("num_cons", "num_vars", "num_io", "nnz", "num_gens"), [x.value for x in v]))

    def digest(self) -> int:
        d = (C.c_uint8 * 32)()
        _check(nova_lib.vdf_nova_pp_digest(self.handle, d))
        return int.from_bytes(bytes(d), "little")

    def segment(self) -> Tuple[int, int]:
        """(first variable, count) of the primary witness's run that the GPU fills: the MinRoot rounds."""
        b, n = C.c_uint64(), C.c_uint64()
        _check(nova_lib.vdf_nova_pp_segment(self.handle, C.byref(b), C.byref(n)))
        return b.value, n.value

    def early_rows(self) -> Tuple[int, int]:
        """(first constraint, count) of the primary rows whose share of T and comm_T a step makes ahead of the rest."""
        b, n = C.c_uint64(), C.c_uint64()
        _check(nova_lib.vdf_nova_pp_early_rows(self.handle, C.byref(b), C.byref(n)))
        return b.value, n.value

    def set_verify_multi(self, n: int) -> None:
        """vdf_nova_pp_set_verify_multi: how many proofs' M(r_x, r_y) one pass over a side's shape evaluates in
        verify_compressed_batch (1..64), or 0 for the per-proof device sequence of the single verifier.  Verdicts do not depend on
        it; a verifier short of device memory lowers it (a point holds its two eq tables meanwhile)."""
        _check(nova_lib.vdf_nova_pp_set_verify_multi(self.handle, n))

    @property
    def verify_multi(self) -> int:
        return int(nova_lib.vdf_nova_pp_verify_multi(self.handle))

    def verify_multi_stats(self) -> Tuple[int, int, int]:
        """(passes launched, points evaluated, points whose comparison failed) since the set was made."""
        out = (_u64 * 3)()
        _check(nova_lib.vdf_nova_pp_verify_multi_stats(self.handle, out))
        return int(out[0]), int(out[1]), int(out[2])

    def set_verify_ro_device(self, min_count: int) -> None:
        """vdf_nova_pp_set_verify_ro_device: from how many entries on verify_aggregate_device / verify_aggregate_wire make an
        aggregate's per-entry Poseidon hashes by vdf_ro_hash_batch on the device; 0 (the default): always on the host.  Verdicts
        do not depend on it."""
        _check(nova_lib.vdf_nova_pp_set_verify_ro_device(self.handle, min_count))

    @property
    def verify_ro_device(self) -> int:
        return int(nova_lib.vdf_nova_pp_verify_ro_device(self.handle))

    def set_verify_ro_block_device(self, min_count: int) -> None:
        """vdf_nova_pp_set_verify_ro_block_device: the same choice for a set made under another RO block (family 1) -- from how many
        entries on the per-entry hashes are made by vdf_ro_hash_batch_block; 0 (the default): on the host.  A separate switch: a
        default-block set ignores it, and set_verify_ro_device keeps its meaning.  Verdicts do not depend on it."""
        _check(nova_lib.vdf_nova_pp_set_verify_ro_block_device(self.handle, min_count))

    @property
    def verify_ro_block_device(self) -> int:
        return int(nova_lib.vdf_nova_pp_verify_ro_block_device(self.handle))

    def verify_ro_stats(self) -> Tuple[int, int]:
        """(hashes made on the device, launches) since the set was made."""
        out = (_u64 * 2)()
        _check(nova_lib.vdf_nova_pp_verify_ro_stats(self.handle, out))
        return int(out[0]), int(out[1])

    def stencil(self) -> int:
        """4 / 3: the early rows run as the MinRoot stencil (reference / bound rounds), 5: as the forward circuit's stencil,
        6: as the forward circuit's in lanes, 7: a custom circuit's periodic rows from their description, 0: through the sparse kernel."""
        return int(nova_lib.vdf_nova_pp_stencil(self.handle))

    def periodic_rows(self) -> "dict | None":
        """A custom circuit's periodic vdf_cs_repeat rows as the parameters found them (whatever the tuning says about using them):
        dict(row_begin, row_count, lead, terms_per_rep), or None."""
        v = [C.c_uint64() for _ in range(4)]
        if not nova_lib.vdf_nova_pp_periodic_rows(self.handle, *[C.byref(x) for x in v]):
            return None
        return dict(zip(("row_begin", "row_count", "lead", "terms_per_rep"), [x.value for x in v]))

    def repeat_rows(self) -> "Tuple[int, int, int] | None":
        """(row_begin, n_cons, t) of a custom circuit's vdf_cs_repeat: repetition j, constraint c is row row_begin + j * n_cons + c;
        None without a repeat.  Does not depend on the rows being periodic."""
        b, n, t = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        if not nova_lib.vdf_nova_pp_repeat_rows(self.handle, C.byref(b), C.byref(n), C.byref(t)):
            return None
        return b.value, n.value, t.value

    def repeat_lanes(self) -> int:
        """The lanes of a custom circuit's repeat (1 for ConstraintSystem.repeat); 0 without a repeat.  Lane l, repetition j,
        constraint c is row row_begin + (l * t + j) * n_cons + c of repeat_rows()."""
        n = C.c_uint64(0)
        nova_lib.vdf_nova_pp_repeat_lanes(self.handle, C.byref(n))
        return n.value

    def field(self) -> int:
        """The orientation: the primary circuit's field, the VDF's -- FIELD_FQ (PallasVDF, G1 = Pallas) or FIELD_FP (VestaVDF, G1 = Vesta)."""
        return int(nova_lib.vdf_nova_pp_field(self.handle))

    def lanes(self) -> int:
        """evaluations a step advances: 1 for every kind but CIRCUIT_MINROOT_FORWARD_LANES"""
        return int(nova_lib.vdf_nova_pp_lanes(self.handle))

    def ro(self) -> dict:
        """The random oracle's parameter block this set was made under (vdf_nova_pp_ro)."""
        r = RoParams()
        _check(nova_lib.vdf_nova_pp_ro(self.handle, C.byref(r)))
        return r.as_dict()

    def tuning(self) -> dict:
        t = NovaTuning()
        _check(nova_lib.vdf_nova_pp_tuning(self.handle, C.byref(t)))
        return t.as_dict()

    def setup_ms(self) -> dict:
        """Wall-clock of the stages of the public_params call that made this set (vdf_nova_pp_setup_ms)."""
        ms = (C.c_double * 7)()
        _check(nova_lib.vdf_nova_pp_setup_ms(self.handle, C.byref(ms)))
        return dict(zip(("shapes_and_digest_host", "shapes_to_device", "generators", "fixed_base_tables", "digit_tables", "other", "total"),
                        [float(x) for x in ms]))

    def memory(self) -> dict:
        """HBM held per side (bytes): generators, fixed-base table, digit table; `skipped` = sides whose digit table did not fit."""
        g, t, d = (np.zeros(2, dtype="<u8") for _ in range(3))
        sk = C.c_uint()
        _check(nova_lib.vdf_nova_pp_memory(self.handle, g.ctypes.data, t.ctypes.data, d.ctypes.data, C.byref(sk)))
        return {"gens_bytes": g.tolist(), "table_bytes": t.tolist(), "digit_table_bytes": d.tolist(), "digit_tables_skipped": sk.value}

    def free(self) -> None:
        if self.handle and self.ctx.handle:      # a dead context took the device memory with it (see hip.Bases.free)
            for proof in list(self._proofs):     # a proof holds device buffers of this context and points at pp
                proof.free()
            nova_lib.vdf_nova_pp_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def public_params(ctx: Context, num_iters_per_step: int, circuit_kind: int = CIRCUIT_MINROOT_REFERENCE,
                  gens_family: int = GENS_TRY_AND_INCREMENT, flags: int = 0, tuning: "NovaTuning | None" = None,
                  ro: "RoParams | None" = None, field: int = FIELD_FQ, **tune) -> NovaVDFPublicParams:      # :232-237
    """`tuning` / keyword fields of vdf_nova_tuning (e.g. digit_window=12, early_rows=0): vdf_nova_public_params_tuned;
    `ro`: the random oracle's parameter block (ro_preset): vdf_nova_public_params_ro; `field`: the orientation, the field of
    the chains these parameters prove (FIELD_FQ: PallasVDF, the default; FIELD_FP: VestaVDF): vdf_nova_public_params_field."""
    h = C.c_void_p()
    if field != FIELD_FQ:
        t = tuning if tuning is not None else tuning_default()
        for k, v in tune.items():
            if k not in dict(NovaTuning._fields_):
                raise KeyError(k)
            setattr(t, k, int(v))
        t.flags |= flags
        _check(nova_lib.vdf_nova_public_params_field(ctx.handle, field, num_iters_per_step, circuit_kind, 1, gens_family, _ro_ptr(ro),
                                                     C.byref(t), C.byref(h)))
    elif ro is not None:
        t = tuning if tuning is not None else tuning_default()
        for k, v in tune.items():
            if k not in dict(NovaTuning._fields_):
                raise KeyError(k)
            setattr(t, k, int(v))
        t.flags |= flags
        _check(nova_lib.vdf_nova_public_params_ro(ctx.handle, num_iters_per_step, circuit_kind, gens_family, C.byref(ro), C.byref(t), C.byref(h)))
    elif tuning is not None or tune:
        t = tuning if tuning is not None else tuning_default()
        for k, v in tune.items():
            if k not in dict(NovaTuning._fields_):
                raise KeyError(k)
            setattr(t, k, int(v))
        t.flags |= flags
        _check(nova_lib.vdf_nova_public_params_tuned(ctx.handle, num_iters_per_step, circuit_kind, gens_family, C.byref(t), C.byref(h)))
    else:
        _check(nova_lib.vdf_nova_public_params_flags(ctx.handle, num_iters_per_step, circuit_kind, gens_family, flags, C.byref(h)))
    pp = NovaVDFPublicParams(ctx, h.value, num_iters_per_step)
    pp.circuit_kind = circuit_kind
    return pp


def public_params_lanes(ctx: Context, num_iters_per_step: int, lanes: int, gens_family: int = GENS_TRY_AND_INCREMENT, flags: int = 0,
                        tuning: "NovaTuning | None" = None, ro: "RoParams | None" = None, field: int = FIELD_FQ, **tune) -> NovaVDFPublicParams:
    """Parameters of the forward circuit in `lanes` lanes (vdf_nova_public_params_lanes); lanes = 1 gives exactly
    public_params(ctx, t, CIRCUIT_MINROOT_FORWARD).  z0 and zi of proofs under them have 3 * lanes elements.  `field`: the
    orientation (public_params)."""
    h = C.c_void_p()
    t = tuning if tuning is not None else tuning_default()
    for k, v in tune.items():
        if k not in dict(NovaTuning._fields_):
            raise KeyError(k)
        setattr(t, k, int(v))
    t.flags |= flags
    if field == FIELD_FQ:
        _check(nova_lib.vdf_nova_public_params_lanes(ctx.handle, num_iters_per_step, lanes, gens_family, _ro_ptr(ro), C.byref(t), C.byref(h)))
    else:
        _check(nova_lib.vdf_nova_public_params_field(ctx.handle, field, num_iters_per_step, CIRCUIT_MINROOT_FORWARD_LANES, lanes, gens_family,
                                                     _ro_ptr(ro), C.byref(t), C.byref(h)))
    pp = NovaVDFPublicParams(ctx, h.value, num_iters_per_step)
    pp.circuit_kind = CIRCUIT_MINROOT_FORWARD if lanes == 1 else CIRCUIT_MINROOT_FORWARD_LANES
    pp.arity = 3 * lanes
    return pp


def shape_digest_lanes(t: int, lanes: int, gens_family: int = 1, ro: "RoParams | None" = None):
    """shape_digest for the forward circuit in `lanes` lanes (host only)."""
    d = (C.c_uint8 * 32)()
    sizes = np.zeros((2, 3), dtype="<u8")
    _check(nova_lib.vdf_nova_shape_digest_lanes(_ro_ptr(ro), t, lanes, gens_family, d, sizes.ctypes.data))
    return int.from_bytes(bytes(d), "little"), sizes.tolist()


def shape_stencil_lanes(t: int, lanes: int):
    """(6, or 5 for one lane, or 0; first early row; early rows; first round variable) -- host only, as shape_stencil."""
    b, n, s_ = C.c_uint64(), C.c_uint64(), C.c_uint64()
    code = nova_lib.vdf_nova_shape_stencil_lanes(t, lanes, C.byref(b), C.byref(n), C.byref(s_))
    if code < 0:
        _check(-code)
    return code, b.value, n.value, s_.value


def shape_export_lanes(t: int, lanes: int, side: int = 0):
    """shape_export for the forward circuit in `lanes` lanes (host only)."""
    nnz = np.zeros(3, dtype="<u8")
    _check(nova_lib.vdf_nova_shape_export_lanes(t, lanes, side, nnz.ctypes.data, None, None, None))
    mats = [(np.zeros(int(z), dtype=np.uint32), np.zeros(int(z), dtype=np.uint32), np.zeros((int(z), 4), dtype="<u8")) for z in nnz]
    arr = lambda k: (C.c_void_p * 3)(*[m[k].ctypes.data for m in mats])
    _check(nova_lib.vdf_nova_shape_export_lanes(t, lanes, side, nnz.ctypes.data, arr(0), arr(1), arr(2)))
    return mats


def aug_synthesize_lanes(t: int, lanes: int, inputs: AugInputs, z0: Sequence[bytes], zi: Sequence[bytes], results: Sequence[State],
                         inps: Sequence[State], cap: int = 1 << 16, ro=None):
    """The primary augmented circuit around the forward circuit in lanes, synthesised on the host: (W, X, z_next, num_cons).
    z0 / zi: 3 * lanes elements (those of `inputs` are ignored); results / inps: one State per lane."""
    W = np.zeros((cap, 4), dtype="<u8")
    X, zn = np.zeros((2, 4), dtype="<u8"), np.zeros((3 * lanes, 4), dtype="<u8")
    nv, nc = C.c_size_t(), C.c_size_t()
    res = b"".join(s.x + s.y + s.i for s in results)
    inp = b"".join(s.x + s.y + s.i for s in inps)
    if len(z0) != 3 * lanes or len(zi) != 3 * lanes or len(res) != 96 * lanes or len(inp) != 96 * lanes:
        raise ValueError("3 * lanes elements of z0 and zi, one state per lane")
    _check(nova_lib.vdf_nova_aug_synthesize_lanes(_ro_ptr(ro), t, lanes, C.addressof(inputs), _zn(z0), _zn(zi), res, inp, W.ctypes.data, cap,
                                                  C.byref(nv), C.byref(nc), X.ctypes.data, zn.ctypes.data))
    return W[:nv.value].copy(), X, zn, nc.value


class Circuits:
    """Vec<InverseMinRootCircuit<G1>> in proving order (already reversed, :294)."""

    def __init__(self, handle: int, t: int):
        self.handle, self.t = handle, t

    def __len__(self) -> int:
        return nova_lib.vdf_nova_circuits_len(self.handle)

    def field(self) -> int:
        """the chain's field (FIELD_FQ / FIELD_FP): what its evaluator, counters, push checks and walks run over"""
        return int(nova_lib.vdf_nova_circuits_field(self.handle))

    def upload(self, ctx: Context) -> None:
        """Move the forward traces into HBM (an input of proving; outside the timed region)."""
        _check(nova_lib.vdf_nova_circuits_upload(ctx.handle, self.handle))
        self._ctx = ctx          # keep the context alive until the traces are freed ...
        ctx._children.add(self)  # ... and let it free them first if it is closed earlier

    def materialize(self, ctx: Context, first: int = 0, count: Optional[int] = None, wait: bool = True) -> List[int]:
        """Checkpoint circuits: build the device traces of circuits [first, first + count) by inverse walks on the GPU.  Returns
        the flags per step (1 = a walk missed its checkpoint; all 0 with wait=False); raises VdfError when any missed."""
        count = len(self) - first if count is None else count
        bad = (C.c_int * max(count, 1))()
        self._ctx = ctx
        ctx._children.add(self)
        rc = nova_lib.vdf_nova_circuits_materialize(ctx.handle, self.handle, first, count, 1 if wait else 0, bad)
        self.last_bad = list(bad)[:count]
        _check(rc)
        return self.last_bad

    def release(self, first: int = 0, count: Optional[int] = None) -> None:
        count = len(self) - first if count is None else count
        _check(nova_lib.vdf_nova_circuits_release(self.handle, first, count))

    def memory(self) -> Tuple[int, int]:
        """(circuits with a device trace, bytes of device memory their traces hold)"""
        n, b = C.c_size_t(0), C.c_uint64(0)
        _check(nova_lib.vdf_nova_circuits_memory(self.handle, C.byref(n), C.byref(b)))
        return n.value, b.value

    def host_bytes(self) -> int:
        """bytes of host memory held in traces and checkpoints"""
        b = C.c_uint64(0)
        _check(nova_lib.vdf_nova_circuits_host_bytes(self.handle, C.byref(b)))
        return b.value

    def trace_ptr(self, k: int) -> Optional[int]:
        """device address of circuit k's trace (2 (t + 1) elements), None without one"""
        p = C.c_void_p()
        _check(nova_lib.vdf_nova_circuit_trace(self.handle, k, C.byref(p)))
        return p.value

    def states(self, k: int) -> Tuple[State, State]:
        """(result, input) of circuit k: InverseMinRootCircuit.result / .input (:63-64)."""
        r, i = _State(), _State()
        _check(nova_lib.vdf_nova_circuit_states(self.handle, k, C.byref(r), C.byref(i)))
        return State._from_c(r), State._from_c(i)

    def free(self) -> None:
        ctx = getattr(self, "_ctx", None)
        if self.handle and (ctx is None or ctx.handle):      # uploaded traces need a live context to be released
            nova_lib.vdf_nova_circuits_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def custom_chain_slices(every: int, launch_rounds: int = 0):
    """The launches vdf_nova_custom_chain_materialize cuts the walks of a window into, by the library's own arithmetic
    (vdf_nova_custom_chain_slice): [(rounds, top, last)], `last` set in the slice that finishes the walks."""
    out, done = [], 0
    while done < every:
        now, top, last = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        _check(nova_lib.vdf_nova_custom_chain_slice(every, launch_rounds, done, 0, C.byref(now), C.byref(top), C.byref(last)))
        out.append((now.value, top.value, bool(last.value)))
        done += now.value
    return out


def custom_chain_window_host(field: int, walk_tape: RoundTape, inv, t: int, every: int, checkpoints: np.ndarray, first: int, count: int,
                             j_base: int = 0, launch_rounds: int = 0):
    """Host only: the window CustomChain.materialize(first, count, launch_rounds=...) builds, by the same sequence of calls over the
    host restatement (walk_tape_eval): (traces uint64[count * (t + 1) * n_adv, 4], the walks' landings, ok int32[count * t / every]).
    checkpoints: the chain's, uint64[(steps * t / every + 1) * n_adv, 4]."""
    na, per = walk_tape.c.n_adv, t // every
    cp = np.ascontiguousarray(checkpoints, dtype="<u8").reshape(-1, na * 4)
    walks = count * per
    entries = cp[first * per + 1: first * per + 1 + walks].copy()
    expect = cp[first * per: first * per + walks].copy()
    trace = np.zeros((count * (t + 1) * na, 4), dtype="<u8")
    ok = np.zeros(walks, dtype="<i4")
    for rounds, top, last in custom_chain_slices(every, launch_rounds):
        walk_tape_eval(field, walk_tape, inv, entries, walks, rounds, trace, walk_stride=every, top=top, group=per, group_stride=t + 1,
                       j_base=(j_base + first * t) % 2**64, j_group_step=t, heads=last, expect=expect if last else None,
                       ok=ok if last else None)
    return trace, entries.reshape(-1, 4), ok


CHAIN_DESCENDING, CHAIN_ASCENDING = 0, 1      # vdf_nova_custom_chain_direction


class CustomChain:
    """vdf_custom_chain: the chain of a custom step circuit, proved from its checkpoints.  The device traces its steps read as
    advice are rebuilt window by window by the chain's walk tape on a side queue (include/vdf_nova.h)."""

    def __init__(self, handle: int, field: int, t: int, every: int, n_adv: int, lanes: int = 1):
        self.handle, self.field, self.t, self.every, self.n_adv, self.lanes = handle, field, t, every, n_adv, lanes

    @staticmethod
    def lanes_from_checkpoints(field: int, walk_tape: RoundTape, inv, t: int, every: int, num_steps: int, lanes: int, checkpoints,
                               lane_stride: Optional[int] = None, j_base=None, forward: bool = False) -> "CustomChain":
        """`lanes` chains of equal length in one chain object (ConstraintSystem.repeat_lanes): lane l's num_steps * (t // every) + 1
        checkpoints start lane_stride entries (default: exactly that many) after lane l - 1's -- consecutive chains of
        Context.round_tape_eval_batch's output, host array or device tensor / address.  inv: lanes * n_inv elements, j_base: one
        counter per lane (default zeros).  A step's trace is lanes * (t + 1) entries.  forward: `walk_tape` is the chain's FORWARD tape
        (a round without a cheap inverse): an ascending chain, its walks start below their interval and land above it."""
        per_lane = num_steps * (t // every) + 1 if every and t % every == 0 else 0
        lane_stride = per_lane if lane_stride is None else lane_stride
        inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
        jb = np.ascontiguousarray([0] * max(lanes, 1) if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
        if 0 < lanes <= 16 and (inv.shape[0] < lanes * walk_tape.c.n_inv or jb.size < lanes):
            raise ValueError("inv or j_base shorter than the lanes read")
        if isinstance(checkpoints, np.ndarray):
            checkpoints = np.ascontiguousarray(checkpoints, dtype="<u8")
            if per_lane and 0 < lanes <= 16 and lane_stride >= per_lane and \
                    checkpoints.size < 4 * ((lanes - 1) * lane_stride + per_lane) * walk_tape.c.n_adv:
                raise ValueError("checkpoints shorter than the lanes read")
        h = C.c_void_p()
        make = nova_lib.vdf_nova_custom_chain_lanes_from_checkpoints_forward if forward else nova_lib.vdf_nova_custom_chain_lanes_from_checkpoints
        _check(make(field, C.addressof(walk_tape.c), inv.ctypes.data if walk_tape.c.n_inv else None, t, every, num_steps, lanes,
                    _ptr(checkpoints), lane_stride, jb.ctypes.data, C.byref(h)))
        return CustomChain(h.value, field, t, every, walk_tape.c.n_adv, lanes)

    @staticmethod
    def from_checkpoints(field: int, walk_tape: RoundTape, inv, t: int, every: int, num_steps: int, checkpoints, j_base: int = 0,
                         forward: bool = False) -> "CustomChain":
        """checkpoints: num_steps * (t // every) + 1 entries of n_adv elements in forward order -- a uint64[., 4] array (host), or a
        device tensor / address (downloaded once).  inv: the walk tape's loop-invariant values, host.  forward: `walk_tape` is the
        chain's FORWARD tape (an ascending chain: rounds without a cheap inverse); j_base means the same number either way."""
        inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
        if inv.shape[0] < walk_tape.c.n_inv:
            raise ValueError("inv shorter than the tape reads")
        if isinstance(checkpoints, np.ndarray):
            checkpoints = np.ascontiguousarray(checkpoints, dtype="<u8")
            if every and t % every == 0 and checkpoints.size < 4 * (num_steps * (t // every) + 1) * walk_tape.c.n_adv:
                raise ValueError("checkpoints shorter than num_steps * (t / every) + 1 entries")
        h = C.c_void_p()
        make = nova_lib.vdf_nova_custom_chain_from_checkpoints_forward if forward else nova_lib.vdf_nova_custom_chain_from_checkpoints
        _check(make(field, C.addressof(walk_tape.c), inv.ctypes.data if walk_tape.c.n_inv else None, t, every, num_steps, _ptr(checkpoints),
                    j_base % 2**64, C.byref(h)))
        return CustomChain(h.value, field, t, every, walk_tape.c.n_adv)

    @staticmethod
    def begin(field: int, tape: RoundTape, direction: int, inv, t: int, initial, lanes: int = 1, j_base=None) -> "CustomChain":
        """An EMPTY chain that stands on `initial` (lanes * n_adv elements: entry 0 of every lane) and grows by one step per
        push_checkpoints / push_advice.  tape: the walk tape (CHAIN_DESCENDING) or the chain's forward tape (CHAIN_ASCENDING)."""
        inv = np.ascontiguousarray(inv if inv is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
        jb = np.ascontiguousarray([0] * max(lanes, 1) if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
        initial = np.ascontiguousarray(initial, dtype="<u8").reshape(-1, 4)
        if 0 < lanes <= 16 and (inv.shape[0] < lanes * tape.c.n_inv or jb.size < lanes or initial.shape[0] < lanes * tape.c.n_adv):
            raise ValueError("inv, j_base or initial shorter than the lanes read")
        h = C.c_void_p()
        _check(nova_lib.vdf_nova_custom_chain_begin(field, C.addressof(tape.c), direction, inv.ctypes.data if tape.c.n_inv else None, t, lanes,
                                                    initial.ctypes.data, jb.ctypes.data, C.byref(h)))
        return CustomChain(h.value, field, t, 0, tape.c.n_adv, lanes)

    def push_checkpoints(self, every: int, cps, lane_stride: Optional[int] = None) -> None:
        """One more step from every lane's t // every + 1 checkpoints, lane l's lane_stride entries (default: exactly that many)
        after lane l - 1's; a uint64[., 4] array (host) or a device tensor / address.  Entry 0 of every lane must be the chain's end."""
        per_lane = self.t // every + 1 if every and self.t % every == 0 else 0
        lane_stride = per_lane if lane_stride is None else lane_stride
        if isinstance(cps, np.ndarray):
            cps = np.ascontiguousarray(cps, dtype="<u8")
            if per_lane and lane_stride >= per_lane and cps.size < 4 * ((self.lanes - 1) * lane_stride + per_lane) * self.n_adv:
                raise ValueError("checkpoints shorter than the lanes read")
        _check(nova_lib.vdf_nova_custom_chain_push_checkpoints(self.handle, every, _ptr(cps), lane_stride))
        self.every = every

    def push_advice(self, advice, lane_stride: Optional[int] = None) -> None:
        """One more step from every lane's whole trace, t + 1 entries each (a host uint64[., 4] array), lane l's lane_stride entries
        (default t + 1) after lane l - 1's.  The chain keeps a host copy until the step is released."""
        lane_stride = self.t + 1 if lane_stride is None else lane_stride
        advice = np.ascontiguousarray(advice, dtype="<u8")
        if lane_stride >= self.t + 1 and advice.size < 4 * ((self.lanes - 1) * lane_stride + self.t + 1) * self.n_adv:
            raise ValueError("advice shorter than the lanes read")
        _check(nova_lib.vdf_nova_custom_chain_push_advice(self.handle, advice.ctypes.data, lane_stride))

    def __len__(self) -> int:
        return nova_lib.vdf_nova_custom_chain_len(self.handle)

    @property
    def direction(self) -> int:
        """CHAIN_DESCENDING (a walk tape) or CHAIN_ASCENDING (a forward tape)"""
        return nova_lib.vdf_nova_custom_chain_direction(self.handle)

    def launch_rounds(self, asked: int = 0) -> int:
        """the rounds per launch a job of this chain runs with when `asked` is requested (an ascending chain lowers it to its bound)"""
        out = C.c_uint64(0)
        _check(nova_lib.vdf_nova_custom_chain_launch_rounds(self.handle, asked, C.byref(out)))
        return out.value

    def set_launch_rounds(self, launch_rounds: int) -> None:
        """the rounds per launch of the jobs whose caller asks for 0, prove_recursively_custom's among them (0: the default)"""
        _check(nova_lib.vdf_nova_custom_chain_set_launch_rounds(self.handle, launch_rounds))

    def materialize(self, ctx: Context, first: int = 0, count: Optional[int] = None, wait: bool = True, launch_rounds: int = 0) -> List[int]:
        """Build the device traces of steps [first, first + count) by walks on the GPU, at most launch_rounds rounds per launch
        (0: 1,024).  Returns the flags per step (1 = a walk missed its checkpoint; all 0 with wait=False); raises VdfError when
        any missed."""
        count = len(self) - first if count is None else count
        bad = (C.c_int * max(count, 1))()
        self._ctx = ctx
        ctx._children.add(self)
        rc = nova_lib.vdf_nova_custom_chain_materialize(ctx.handle, self.handle, first, count, 1 if wait else 0, launch_rounds, bad)
        self.last_bad = list(bad)[:count]
        _check(rc)
        return self.last_bad

    def release(self, first: int = 0, count: Optional[int] = None) -> None:
        count = len(self) - first if count is None else count
        _check(nova_lib.vdf_nova_custom_chain_release(self.handle, first, count))

    def memory(self) -> Tuple[int, int]:
        """(steps with a device trace, bytes of device memory the traces hold)"""
        n, b = C.c_size_t(0), C.c_uint64(0)
        _check(nova_lib.vdf_nova_custom_chain_memory(self.handle, C.byref(n), C.byref(b)))
        return n.value, b.value

    def host_bytes(self) -> int:
        """bytes of host memory held in the tape, inv and the checkpoints"""
        b = C.c_uint64(0)
        _check(nova_lib.vdf_nova_custom_chain_host_bytes(self.handle, C.byref(b)))
        return b.value

    def advice(self, k: int) -> Optional[int]:
        """device address of step k's trace (lanes * (t + 1) * n_adv elements), None without one; pending walks over it are finished first"""
        p = C.c_void_p()
        _check(nova_lib.vdf_nova_custom_chain_advice(self.handle, k, C.byref(p)))
        return p.value

    def free(self) -> None:
        ctx = getattr(self, "_ctx", None)
        if self.handle and (ctx is None or ctx.handle):      # device traces need a live context to be released
            nova_lib.vdf_nova_custom_chain_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class InverseMinRootCircuit:      # src/nova/proof.rs:57-66, :239-299
    arity = 3                     # :83-85

    @staticmethod
    def eval_and_make_circuits(v: MinRootVDF, num_iters_per_step: int, num_steps: int,
                               initial_state: State) -> Tuple[List[bytes], Circuits]:   # :262-299
        if num_steps <= 0:
            raise AssertionError("num_steps > 0")                                       # :268
        z0 = (_Fe * 3)()
        h = C.c_void_p()
        if v.FIELD == FIELD_FQ:
            _check(nova_lib.vdf_nova_eval_and_make_circuits(int(v.eval_mode), num_iters_per_step, num_steps,
                                                            C.byref(initial_state._c()), C.byref(z0), C.byref(h)))
        else:                                                                           # the field comes from v: VestaVDF gives Fp
            _check(nova_lib.vdf_nova_eval_and_make_circuits_field(v.FIELD, int(v.eval_mode), num_iters_per_step, num_steps,
                                                                  C.byref(initial_state._c()), C.byref(z0), C.byref(h)))
        return [bytes(z0[k]) for k in range(3)], Circuits(h.value, num_iters_per_step)

    @staticmethod
    def from_checkpoints(t: int, every: int, num_steps: int, states: Sequence[State], field: int = FIELD_FQ) -> Tuple[List[bytes], Circuits]:
        """The circuits of a chain evaluated elsewhere, from its states every `every` rounds in forward order
        (num_steps * (t // every) + 1 of them, e.g. MinRootVDF.eval_checkpoints): no trace is held; Circuits.materialize, or
        prove_recursively by itself, rebuilds the traces on the GPU window by window."""
        if every > 0 and t % every == 0 and num_steps > 0 and len(states) != num_steps * (t // every) + 1:
            raise ValueError("num_steps * (t // every) + 1 states expected")
        raw = b"".join(s.x + s.y + s.i for s in states)
        buf = (C.c_char * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        z0 = (_Fe * 3)()
        h = C.c_void_p()
        if field == FIELD_FQ:
            _check(nova_lib.vdf_nova_circuits_from_checkpoints(t, every, num_steps, buf, C.byref(z0), C.byref(h)))
        else:
            _check(nova_lib.vdf_nova_circuits_from_checkpoints_field(field, t, every, num_steps, buf, C.byref(z0), C.byref(h)))
        return [bytes(z0[k]) for k in range(3)], Circuits(h.value, t)


class ForwardCircuits(Circuits):
    """A chain of forward step circuits (CIRCUIT_MINROOT_FORWARD) that grows while the chain is evaluated: circuit k is the
    k-th step pushed.  Push and release between prove_steps, never during one (include/vdf_nova.h)."""

    @staticmethod
    def begin(t: int, initial_state: State, field: int = FIELD_FQ) -> Tuple[List[bytes], "ForwardCircuits"]:
        """(z0 = the initial state, an empty chain); `field`: the chain's field"""
        z0 = (_Fe * 3)()
        h = C.c_void_p()
        if field == FIELD_FQ:
            _check(nova_lib.vdf_nova_circuits_forward_begin(t, C.byref(initial_state._c()), C.byref(z0), C.byref(h)))
        else:
            _check(nova_lib.vdf_nova_circuits_forward_begin_field(field, t, C.byref(initial_state._c()), C.byref(z0), C.byref(h)))
        return [bytes(z0[k]) for k in range(3)], ForwardCircuits(h.value, t)

    def push_trace(self, trace_xy: np.ndarray) -> None:
        """Appends a step from its host trace, (x, y) of states 0..t as MinRootVDF.eval_with_trace returns it."""
        tr = np.ascontiguousarray(trace_xy, dtype="<u8").reshape(-1, 4)
        if tr.shape[0] != 2 * (self.t + 1):
            raise ValueError("2 (t + 1) elements expected")
        _check(nova_lib.vdf_nova_circuits_push_trace(self.handle, tr.ctypes.data))

    def push_checkpoints(self, every: int, states: Sequence[State]) -> None:
        """Appends a step from its t // every + 1 states every `every` rounds; materialize rebuilds its trace on the GPU."""
        if every > 0 and self.t % every == 0 and len(states) != self.t // every + 1:
            raise ValueError("t // every + 1 states expected")
        raw = b"".join(s.x + s.y + s.i for s in states)
        buf = (C.c_char * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        _check(nova_lib.vdf_nova_circuits_push_checkpoints(self.handle, every, buf))


class LaneCircuits(Circuits):
    """A forward chain in lanes (CIRCUIT_MINROOT_FORWARD_LANES): every step advances `lanes` evaluations by t rounds.  One lane
    is a forward chain.  Push and release between prove_steps, never during one (include/vdf_nova.h)."""

    @staticmethod
    def begin(t: int, initials: Sequence[State], field: int = FIELD_FQ) -> Tuple[List[bytes], "LaneCircuits"]:
        """(z0 = the lanes' initial states flattened, an empty chain); `field`: the chains' field"""
        L = len(initials)
        z0 = (_Fe * (3 * max(L, 1)))()
        raw = b"".join(s.x + s.y + s.i for s in initials) or bytes(96)
        h = C.c_void_p()
        if field == FIELD_FQ:
            _check(nova_lib.vdf_nova_circuits_lanes_begin(t, L, raw, z0, C.byref(h)))
        else:
            _check(nova_lib.vdf_nova_circuits_lanes_begin_field(field, t, L, raw, z0, C.byref(h)))
        c = LaneCircuits(h.value, t)
        c.lanes = L
        return [bytes(z0[k]) for k in range(3 * L)], c

    def push_traces(self, traces, lane_stride: Optional[int] = None) -> None:
        """Appends a step from the lanes' host traces: a sequence of `lanes` arrays of 2 (t + 1) elements, or one array of
        lanes x 2 lane_stride elements."""
        if lane_stride is None:
            lane_stride = self.t + 1
            tr = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype="<u8").reshape(-1, 4) for x in traces]), dtype="<u8")
        else:
            tr = np.ascontiguousarray(traces, dtype="<u8").reshape(-1, 4)
        if tr.shape[0] < 2 * ((self.lanes - 1) * lane_stride + self.t + 1):
            raise ValueError("lanes traces of 2 (t + 1) elements expected")
        _check(nova_lib.vdf_nova_circuits_push_traces(self.handle, tr.ctypes.data, lane_stride))

    def push_checkpoints(self, every: int, states, lane_stride: Optional[int] = None) -> None:
        """Appends a step from every lane's t // every + 1 states: a sequence of `lanes` sequences of State, or (with lane_stride)
        one uint64 array of states laid out as vdf_minroot_eval_batch writes them, lane l's at states[l * lane_stride]."""
        if lane_stride is None:
            lane_stride = len(states[0])
            raw = b"".join(s.x + s.y + s.i for lane in states for s in lane)
            if any(len(lane) != lane_stride for lane in states) or len(states) != self.lanes:
                raise ValueError("lanes runs of equally many states expected")
            buf = (C.c_char * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
            _check(nova_lib.vdf_nova_circuits_push_checkpoints_lanes(self.handle, every, buf, lane_stride))
        else:
            arr = np.ascontiguousarray(states, dtype="<u8")
            _check(nova_lib.vdf_nova_circuits_push_checkpoints_lanes(self.handle, every, arr.ctypes.data, lane_stride))

    def lane_states(self, k: int, lane: int) -> Tuple[State, State]:
        """(result, input) of lane `lane` of circuit k"""
        r, i = _State(), _State()
        _check(nova_lib.vdf_nova_circuit_lane_states(self.handle, k, lane, C.byref(r), C.byref(i)))
        return State._from_c(r), State._from_c(i)


class StreamStats(C.Structure):   # vdf_nova_stream_stats
    _fields_ = [("eval_ms", C.c_double), ("after_eval_ms", C.c_double), ("max_backlog", C.c_uint64), ("steps", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class _CustomStream(C.Structure):  # vdf_nova_custom_stream
    _fields_ = [("forward_tape", C.c_void_p), ("inv", C.c_void_p), ("walk_tape", C.c_void_p), ("walk_inv", C.c_void_p),
                ("t", C.c_uint64), ("every", C.c_uint64), ("lanes", C.c_size_t), ("j_base", C.c_void_p)]


class NovaVDFProof:               # enum NovaVDFProof { Recursive, Compressed }, :51-55
    def __init__(self, handle: int, pp: NovaVDFPublicParams):
        self.handle, self.pp = handle, pp
        pp.ctx._children.add(self)
        pp._proofs.add(self)

    @staticmethod
    def prove_recursively(pp: NovaVDFPublicParams, circuits: Circuits, num_iters_per_step: int,
                          z0: Sequence[bytes], window_steps: Optional[int] = None) -> "NovaVDFProof":   # :302-358
        """window_steps: over checkpoint circuits, how many steps' traces one window of inverse walks rebuilds (None: 1 GiB's worth)."""
        h = C.c_void_p()
        if window_steps is None:
            _check(nova_lib.vdf_nova_prove_recursively(pp.handle, circuits.handle, num_iters_per_step, C.byref(_z(z0)), C.byref(h)))
        else:
            _check(nova_lib.vdf_nova_prove_recursively_windowed(pp.handle, circuits.handle, num_iters_per_step, C.byref(_z(z0)),
                                                                window_steps, C.byref(h)))
        return NovaVDFProof(h.value, pp)

    @staticmethod
    def eval_and_prove(pp: NovaVDFPublicParams, v: MinRootVDF, initial_state: State, num_steps: int) -> Tuple["NovaVDFProof", State, dict]:
        """Evaluates num_steps steps from initial_state on a library thread and proves every step as it arrives (forward
        parameters): (the running proof of z0 = initial, zi = final; the final state; vdf_nova_stream_stats as a dict).  The
        evaluator runs the parameters' field, which must be v's (VestaVDF needs public_params(..., field=FIELD_FP))."""
        if nova_lib.vdf_nova_pp_field(pp.handle) != v.FIELD:
            raise VdfError(1, "the parameters' orientation is not the field of this VDF (public_params(..., field=...))")
        h = C.c_void_p()
        fin, st = _State(), StreamStats()
        _check(nova_lib.vdf_nova_eval_and_prove(pp.handle, int(v.eval_mode), C.byref(initial_state._c()), num_steps, C.byref(fin),
                                                C.byref(h), C.addressof(st)))
        return NovaVDFProof(h.value, pp), State._from_c(fin), st.as_dict()

    @staticmethod
    def eval_and_prove_custom(pp: NovaVDFPublicParams, circuit: "StepCircuit", forward_tape: RoundTape, inv, t: int, initial, num_steps: int,
                              z0: Sequence[bytes], every: int = 0, walk_tape: Optional[RoundTape] = None, walk_inv=None, lanes: int = 1,
                              j_base=None) -> Tuple["NovaVDFProof", np.ndarray, dict]:
        """A custom chain proved while it is evaluated (vdf_nova_eval_and_prove_custom): library threads, one per lane, evaluate
        num_steps steps of t rounds from `initial` (lanes * n_adv elements) by forward_tape on the host; this thread is handed the
        steps -- whole traces (every = 0) or checkpoints every `every` rounds, rebuilt on the GPU by walk_tape or, without one, by
        forward_tape itself -- and proves them as they arrive.  `circuit.synthesize` runs on this thread only.  Returns (the running
        proof, the lanes' final entries as uint64[lanes * n_adv, 4], vdf_nova_stream_stats as a dict)."""
        arr = lambda a: np.ascontiguousarray(a if a is not None else np.zeros((0, 4)), dtype="<u8").reshape(-1, 4)
        inv, walk_inv, initial = arr(inv), arr(walk_inv), arr(initial)
        jb = np.ascontiguousarray([0] * max(lanes, 1) if j_base is None else [int(v) % 2**64 for v in j_base], dtype="<u8")
        n_adv = forward_tape.c.n_adv
        if 0 < lanes <= 16 and (inv.shape[0] < lanes * forward_tape.c.n_inv or jb.size < lanes or initial.shape[0] < lanes * n_adv or
                                (walk_tape is not None and walk_inv.shape[0] < lanes * walk_tape.c.n_inv)):
            raise ValueError("inv, walk_inv, j_base or initial shorter than the lanes read")
        s = _CustomStream(C.addressof(forward_tape.c), inv.ctypes.data if forward_tape.c.n_inv else None,
                          C.addressof(walk_tape.c) if walk_tape is not None else None,
                          walk_inv.ctypes.data if walk_tape is not None and walk_tape.c.n_inv else None, t, every, lanes, jb.ctypes.data)
        fin = np.zeros((max(lanes, 1) * n_adv, 4), dtype="<u8")
        h, st = C.c_void_p(), StreamStats()
        rc = nova_lib.vdf_nova_eval_and_prove_custom(pp.handle, C.byref(circuit._c()), C.byref(s), initial.ctypes.data, num_steps, _zn(z0),
                                                     fin.ctypes.data, C.byref(h), C.addressof(st))
        _reraise(circuit)
        _check(rc)
        return NovaVDFProof(h.value, pp), fin, st.as_dict()

    @staticmethod
    def prove_step(pp: NovaVDFPublicParams, proof: "NovaVDFProof | None", circuits: Circuits, k: int,
                   z0: Sequence[bytes]) -> "NovaVDFProof":                              # RecursiveSNARK::prove_step, :342-349
        h = C.c_void_p(proof.handle if proof is not None else None)
        _check(nova_lib.vdf_nova_prove_step(pp.handle, C.byref(h), circuits.handle, k, C.byref(_z(z0))))
        if proof is None:
            return NovaVDFProof(h.value, pp)
        return proof

    def verify(self, pp: NovaVDFPublicParams, num_steps: int, z0: Sequence[bytes], zi: Sequence[bytes]) -> bool:   # :370-387
        ok = C.c_int(0)
        _check(nova_lib.vdf_nova_verify_custom(self.handle, pp.handle, num_steps, _zn(z0), _zn(zi), C.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def prove_step_custom(pp: NovaVDFPublicParams, proof: "NovaVDFProof | None", circuit: "StepCircuit",
                          z0: Sequence[bytes]) -> "NovaVDFProof":
        """prove_step for a host-written primary step circuit (public_params_custom)."""
        h = C.c_void_p(proof.handle if proof is not None else None)
        rc = nova_lib.vdf_nova_prove_step_custom(pp.handle, C.byref(h), C.byref(circuit._c()), _zn(z0))
        _reraise(circuit)
        _check(rc)
        return NovaVDFProof(h.value, pp) if proof is None else proof

    @staticmethod
    def prove_step_custom_chain(pp: NovaVDFPublicParams, proof: "NovaVDFProof | None", circuit: "StepCircuit", chain: "CustomChain", k: int,
                                z0: Sequence[bytes]) -> "NovaVDFProof":
        """prove_step_custom for step k of a chain, k = 0, 1, ... in order: the step's device trace is what the circuit's
        cs.step_advice() answers."""
        h = C.c_void_p(proof.handle if proof is not None else None)
        rc = nova_lib.vdf_nova_prove_step_custom_chain(pp.handle, C.byref(h), C.byref(circuit._c()), chain.handle, k, _zn(z0))
        _reraise(circuit)
        _check(rc)
        return NovaVDFProof(h.value, pp) if proof is None else proof

    @staticmethod
    def prove_recursively_custom(pp: NovaVDFPublicParams, circuit: "StepCircuit", chain: "CustomChain", z0: Sequence[bytes],
                                 window_steps: int = 0, check_steps: bool = False) -> "NovaVDFProof":
        """Every step of the chain, the walks of window w + 1 under the proving of window w (window_steps = 0: 1 GiB's worth).
        check_steps: every step's fresh instance is scanned, and an unsatisfied row ends the call with a VdfError naming it."""
        h = C.c_void_p()
        chain._ctx = pp.ctx
        pp.ctx._children.add(chain)
        rc = nova_lib.vdf_nova_prove_recursively_custom(pp.handle, C.byref(circuit._c()), chain.handle, _zn(z0), window_steps,
                                                        CUSTOM_CHECK_STEPS if check_steps else 0, C.byref(h))
        _reraise(circuit)
        _check(rc)
        return NovaVDFProof(h.value, pp)

    def last_unsat(self) -> Tuple[int, int]:
        """(unsatisfied rows of the LAST step's fresh primary instance, the first of them or 2**64 - 1)"""
        n, r = C.c_uint64(0), C.c_uint64(0)
        _check(nova_lib.vdf_nova_proof_last_unsat(self.handle, C.byref(n), C.byref(r)))
        return n.value, r.value

    def ahead_stats(self) -> Tuple[int, int, int]:
        """(hits, misses, skipped): the steps after the first in which a custom chain's lookahead (tuning custom_ahead) was used,
        discarded, or not attempted; zeros for every other kind of proof."""
        v = [C.c_uint64() for _ in range(3)]
        _check(nova_lib.vdf_nova_proof_ahead_stats(self.handle, *[C.byref(x) for x in v]))
        return v[0].value, v[1].value, v[2].value

    def compress(self, pp: NovaVDFPublicParams) -> "CompressedNovaVDFProof":            # :360-368
        h = C.c_void_p()
        _check(nova_lib.vdf_nova_compress(self.handle, pp.handle, C.byref(h)))
        return CompressedNovaVDFProof(h.value, pp)

    # ---- checkpoint: the running proof as bytes ("VDFRSK01", include/vdf_nova.h) ----
    def serialize(self) -> bytes:
        n = nova_lib.vdf_nova_proof_serialized_size(self.handle)
        buf = (C.c_uint8 * n)()
        _check(nova_lib.vdf_nova_proof_serialize(self.handle, buf, n))
        return bytes(buf)

    @staticmethod
    def deserialize(pp: NovaVDFPublicParams, data: bytes) -> "NovaVDFProof":
        """Rebuilds the device-resident running proof; prove_step continues from it."""
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        h = C.c_void_p()
        _check(nova_lib.vdf_nova_proof_deserialize(pp.handle, buf, len(data), C.byref(h)))
        return NovaVDFProof(h.value, pp)

    # ---- introspection used by the parity tests and the bench ----
    def num_steps(self) -> int:
        return nova_lib.vdf_nova_proof_num_steps(self.handle)

    def instance(self, which: int = INST_RUNNING_PRIMARY) -> dict:
        cw, ce = np.zeros(8, dtype="<u8"), np.zeros(8, dtype="<u8")
        u, X = np.zeros(4, dtype="<u8"), np.zeros((2, 4), dtype="<u8")
        _check(nova_lib.vdf_nova_proof_instance(self.handle, which, cw.ctypes.data, ce.ctypes.data, u.ctypes.data, X.ctypes.data))
        return {"comm_W": cw, "comm_E": ce, "u": u, "X": X}

    def witness(self, which: int = INST_RUNNING_PRIMARY) -> Tuple[np.ndarray, np.ndarray]:
        """Downloads (z = [W | u | X], E) of one of the three instances for parity checks (E is None for the fresh one)."""
        from ._lib import lib
        s = self.pp.sizes(0 if which in (INST_RUNNING_PRIMARY, INST_FRESH_PRIMARY_LAST) else 1)
        dz, dE = C.c_void_p(), C.c_void_p()
        _check(nova_lib.vdf_nova_proof_witness_ptrs(self.handle, which, C.byref(dz), C.byref(dE)))
        z = np.zeros((s["num_vars"] + 3, 4), dtype="<u8")
        self.pp.ctx._check(lib.vdf_dev_memcpy(self.pp.ctx.handle, z.ctypes.data, dz.value, z.nbytes))
        E = None
        if dE.value:
            E = np.zeros((s["num_cons"], 4), dtype="<u8")
            self.pp.ctx._check(lib.vdf_dev_memcpy(self.pp.ctx.handle, E.ctypes.data, dE.value, E.nbytes))
        return z, E

    def zi(self) -> Tuple[np.ndarray, np.ndarray]:
        a, b = np.zeros((getattr(self.pp, "arity", 3), 4), dtype="<u8"), np.zeros((1, 4), dtype="<u8")
        _check(nova_lib.vdf_nova_proof_zi(self.handle, a.ctypes.data, b.ctypes.data))
        return a, b

    def last_step(self) -> dict:
        """By-products of the last prove_step: fresh primary instance, cross-term commitments, fold challenges."""
        raw = np.zeros(8 + 8 + 8 + 8 + 4 + 4, dtype="<u8")
        _check(nova_lib.vdf_nova_proof_last_step(self.handle, raw.ctypes.data))
        return {"comm_W1": raw[0:8], "X1": raw[8:16].reshape(2, 4), "comm_T1": raw[16:24], "comm_T2": raw[24:32],
                "r1": int.from_bytes(raw[32:36].tobytes(), "little"), "r2": int.from_bytes(raw[36:40].tobytes(), "little")}

    def last_step_ms(self) -> dict:
        ms = (C.c_double * 8)()
        _check(nova_lib.vdf_nova_last_step_ms(self.handle, C.byref(ms)))
        return dict(zip(("secondary_nifs", "primary_synthesis", "primary_launch", "primary_wait", "secondary_synthesis", "secondary_launch", "lookahead", "total"), list(ms)))

    def set_kernel_timing(self, flag: bool) -> None:
        """HIP events around every launch of this prover's three queues (include/vdf_nova.h); measure rates with it off."""
        _check(nova_lib.vdf_nova_proof_set_kernel_timing(self.handle, int(flag)))

    def kernel_events(self) -> list:
        """Drains the timed launches: [(queue, kernel, algorithmic bytes, start_ms, end_ms)] on the device's common time line."""
        n = C.c_size_t()
        _check(nova_lib.vdf_nova_proof_kernel_events(self.handle, None, None, 0, C.byref(n)))
        cap = n.value + 64
        ev = np.zeros(cap, dtype=KERNEL_EVENT_DTYPE)
        q = np.zeros(cap, dtype=np.int32)
        _check(nova_lib.vdf_nova_proof_kernel_events(self.handle, ev.ctypes.data, q.ctypes.data, cap, C.byref(n)))
        return [(int(q[i]), ev["name"][i].decode(), float(ev["bytes"][i]), float(ev["start_ms"][i]), float(ev["end_ms"][i]))
                for i in range(n.value)]

    def free(self) -> None:
        if self.handle and self.pp.handle and self.pp.ctx.handle:      # needs live parameters and a live context
            nova_lib.vdf_nova_proof_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CompressedNovaVDFProof:     # NovaVDFProof::Compressed, src/nova/proof.rs:54
    def __init__(self, handle: int, pp: NovaVDFPublicParams):
        self.handle, self.pp = handle, pp
        pp.ctx._children.add(self)
        pp._proofs.add(self)

    def verify(self, pp: NovaVDFPublicParams, num_steps: int, z0: Sequence[bytes], zi: Sequence[bytes]) -> bool:   # :370-387
        ok = C.c_int(0)
        _check(nova_lib.vdf_nova_verify_compressed(self.handle, pp.handle, num_steps, C.cast(_zn(z0), C.POINTER(_Fe * 3)),
                                                   C.cast(_zn(zi), C.POINTER(_Fe * 3)), C.byref(ok)))
        return bool(ok.value)

    def to_bytes(self) -> bytes:
        """The argument in its flat canonical encoding (include/vdf_nova.h)."""
        n = nova_lib.vdf_nova_snark_size(self.handle)
        buf = (C.c_uint8 * n)()
        _check(nova_lib.vdf_nova_snark_bytes(self.handle, buf, n))
        return bytes(buf)

    def set_bytes(self, data: bytes) -> None:
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        _check(nova_lib.vdf_nova_snark_set_bytes(self.handle, buf, len(data)))

    def serialize(self) -> bytes:
        """The whole compressed proof (step chain + argument, 32-byte points): "VDFSNK01", include/vdf_nova.h."""
        n = nova_lib.vdf_nova_snark_serialized_size(self.handle)
        buf = (C.c_uint8 * n)()
        _check(nova_lib.vdf_nova_snark_serialize(self.handle, buf, n))
        return bytes(buf)

    @staticmethod
    def deserialize(pp: NovaVDFPublicParams, data: bytes) -> "CompressedNovaVDFProof":
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        h = C.c_void_p()
        _check(nova_lib.vdf_nova_snark_deserialize(pp.handle, buf, len(data), C.byref(h)))
        return CompressedNovaVDFProof(h.value, pp)

    def free(self) -> None:
        if self.handle and self.pp.handle and self.pp.ctx.handle:
            nova_lib.vdf_nova_snark_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def compress_batch(pp: NovaVDFPublicParams, proofs: Sequence["NovaVDFProof"]) -> list:
    """Compresses many proofs under one parameter set (vdf_nova_compress_batch): one CompressedNovaVDFProof per entry, each
    serialising to what proof.compress(pp) gives; a proof named twice gets two independent copies."""
    n = len(proofs)
    if n == 0:
        return []
    hs = (_vp * n)(*[None if p is None else p.handle for p in proofs])
    out = (_vp * n)()
    _check(nova_lib.vdf_nova_compress_batch(pp.handle, n, hs, out))
    return [CompressedNovaVDFProof(out[q], pp) for q in range(n)]


def verify_compressed_batch(pp: NovaVDFPublicParams, items: Sequence[tuple]) -> list:
    """Verifies many compressed proofs at once (vdf_nova_verify_compressed_batch): items = [(snark, num_steps, z0, zi), ...];
    returns one bool per item, each what snark.verify(pp, num_steps, z0, zi) returns."""
    n = len(items)
    arity = getattr(pp, "arity", 3)
    snarks = (_vp * max(n, 1))(*[it[0].handle for it in items])
    steps = (_sz * max(n, 1))(*[int(it[1]) for it in items])
    for it in items:
        if len(it[2]) != arity or len(it[3]) != arity:
            raise ValueError(f"z0 and zi need {arity} elements each")
    z0 = _zn([v for it in items for v in it[2]] or [bytes(32)])
    zi = _zn([v for it in items for v in it[3]] or [bytes(32)])
    ok = (_i * max(n, 1))()
    all_ok = C.c_int(0)
    _check(nova_lib.vdf_nova_verify_compressed_batch(pp.handle, n, snarks, steps, z0, zi, ok, C.byref(all_ok)))
    return [bool(ok[q]) for q in range(n)]


def _blob_arrays(blobs):
    """(keep-alive buffers, const uint8_t* const in[], size_t len[]) of a list of byte strings"""
    n = len(blobs)
    bufs = [(C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0") for b in blobs]
    ins = (_vp * max(n, 1))(*[C.addressof(b) for b in bufs])
    lens = (_sz * max(n, 1))(*[len(b) for b in blobs])
    return bufs, ins, lens


def deserialize_compressed_batch(pp: NovaVDFPublicParams, blobs: Sequence[bytes]) -> list:
    """Many compressed proofs from their wire bytes, their points decoded on the device (vdf_nova_snark_deserialize_batch):
    [(proof | None, status)] per blob, status the code CompressedNovaVDFProof.deserialize would raise for that blob alone
    (vdf_amd.OK = 0 with the proof)."""
    n = len(blobs)
    bufs, ins, lens = _blob_arrays(blobs)
    out = (_vp * max(n, 1))()
    status = (_i * max(n, 1))()
    _check(nova_lib.vdf_nova_snark_deserialize_batch(pp.handle, n, ins, lens, out, status))
    return [(CompressedNovaVDFProof(out[q], pp) if out[q] else None, int(status[q])) for q in range(n)]


def verify_wire_batch(pp: NovaVDFPublicParams, items: Sequence[tuple]) -> list:
    """Bytes in, verdicts out (vdf_nova_verify_wire_batch): items = [(blob, num_steps, z0, zi), ...]; [(ok, status)] per item.
    A blob that does not decode has ok = False and its code; the others' verdicts are those of verify_compressed_batch over
    singly deserialised proofs, as if that blob were absent."""
    n = len(items)
    arity = getattr(pp, "arity", 3)
    for it in items:
        if len(it[2]) != arity or len(it[3]) != arity:
            raise ValueError(f"z0 and zi need {arity} elements each")
    bufs, ins, lens = _blob_arrays([it[0] for it in items])
    steps = (_sz * max(n, 1))(*[int(it[1]) for it in items])
    z0 = _zn([v for it in items for v in it[2]] or [bytes(32)])
    zi = _zn([v for it in items for v in it[3]] or [bytes(32)])
    ok = (_i * max(n, 1))()
    status = (_i * max(n, 1))()
    all_ok = C.c_int(0)
    _check(nova_lib.vdf_nova_verify_wire_batch(pp.handle, n, ins, lens, steps, z0, zi, ok, status, C.byref(all_ok)))
    res = [(bool(ok[q]), int(status[q])) for q in range(n)]
    assert bool(all_ok.value) == all(o for o, _ in res)
    return res


def verify_batch(pp: NovaVDFPublicParams, items: Sequence[tuple]) -> list:
    """Verifies many running proofs at once (vdf_nova_verify_batch): items = [(proof, num_steps, z0, zi), ...]; returns one
    bool per item, each what proof.verify(pp, num_steps, z0, zi) returns.  The proofs go on proving as if unverified."""
    n = len(items)
    arity = getattr(pp, "arity", 3)
    proofs = (_vp * max(n, 1))(*[None if it[0] is None else it[0].handle for it in items])
    steps = (_sz * max(n, 1))(*[int(it[1]) for it in items])
    for it in items:
        if len(it[2]) != arity or len(it[3]) != arity:
            raise ValueError(f"z0 and zi need {arity} elements each")
    z0 = _zn([v for it in items for v in it[2]] or [bytes(32)])
    zi = _zn([v for it in items for v in it[3]] or [bytes(32)])
    ok = (_i * max(n, 1))()
    all_ok = C.c_int(0)
    _check(nova_lib.vdf_nova_verify_batch(pp.handle, n, proofs, steps, z0, zi, ok, C.byref(all_ok)))
    return [bool(ok[q]) for q in range(n)]


AGGREGATE_MAX = 1024              # VDF_NOVA_AGGREGATE_MAX
WIRE_INSTANCE_BYTES = 160         # sizeof(vdf_wire_instance): comm_W | comm_E | u | X[2]


def _aggregate_statements(pp, num_steps, z0, zi):
    """(count, num_steps, z0, zi) as the aggregate's verifiers take them; the shapes are checked here, before any library call"""
    n = len(num_steps)
    arity = getattr(pp, "arity", 3)
    if len(z0) != n or len(zi) != n or any(len(v) != arity for v in list(z0) + list(zi)):
        raise ValueError(f"z0 and zi need {arity} elements for each of the {n} entries")
    steps = (_sz * max(n, 1))(*[int(v) for v in num_steps])
    z0a = _zn([v for e in z0 for v in e] or [bytes(32)])
    zia = _zn([v for e in zi for v in e] or [bytes(32)])
    return n, steps, z0a, zia


def _wire_instances(instances, comm_TT):
    """the byte arrays of a fold over plain bytes; the lengths are checked here, before any library call"""
    n = len(instances)
    if any(len(b) != WIRE_INSTANCE_BYTES for b in instances) or any(len(b) != 32 for b in comm_TT):
        raise ValueError("instances are 160 bytes, points and the digest 32")
    if n and len(comm_TT) != n - 1:
        raise ValueError("one cross-term commitment per fold")
    inst = (C.c_uint8 * max(160 * n, 1)).from_buffer_copy(b"".join(instances) or b"\0")
    tt = (C.c_uint8 * max(32 * len(comm_TT), 1)).from_buffer_copy(b"".join(comm_TT) or b"\0")
    return n, inst, tt


class AggregateProof:
    """Many running proofs under one parameter set as ONE compressed proof ("vdf-aggregate-v1", include/vdf_nova.h)."""

    def __init__(self, handle: int, pp: NovaVDFPublicParams):
        self.handle, self.pp = handle, pp
        pp.ctx._children.add(self)
        pp._proofs.add(self)

    @property
    def count(self) -> int:
        return int(nova_lib.vdf_nova_aggregate_count(self.handle))

    def verify(self, pp: NovaVDFPublicParams, num_steps: Sequence[int], z0: Sequence[Sequence[bytes]], zi: Sequence[Sequence[bytes]],
               device: bool = False):
        """(ok, bad_entry): one verdict for the whole aggregate; bad_entry = the first entry whose exact checks fail, else -1.
        num_steps, z0, zi: one per entry (z0[k], zi[k]: `arity` elements).  device: the per-entry folds and both accumulators by
        the GPU (vdf_nova_verify_aggregate_device) instead of host point arithmetic; the same verdict either way."""
        n, steps, z0a, zia = _aggregate_statements(pp, num_steps, z0, zi)
        ok, bad = C.c_int(0), C.c_int64(-1)
        call = nova_lib.vdf_nova_verify_aggregate_device if device else nova_lib.vdf_nova_verify_aggregate
        _check(call(self.handle, pp.handle, n, steps, z0a, zia, C.byref(ok), C.byref(bad)))
        return bool(ok.value), int(bad.value)

    def serialize(self) -> bytes:
        """ "VDFAGG01" (include/vdf_nova.h)."""
        n = nova_lib.vdf_nova_aggregate_serialized_size(self.handle)
        buf = (C.c_uint8 * n)()
        _check(nova_lib.vdf_nova_aggregate_serialize(self.handle, buf, n))
        return bytes(buf)

    def free(self) -> None:
        if self.handle and self.pp.handle and self.pp.ctx.handle:
            nova_lib.vdf_nova_aggregate_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def compress_aggregate(pp: NovaVDFPublicParams, proofs: Sequence["NovaVDFProof"]) -> AggregateProof:
    """Folds the running instances of many proofs into one and proves one argument per side (vdf_nova_compress_aggregate).  The
    proofs are left as compress leaves them; a proof named twice is folded twice."""
    n = len(proofs)
    hs = (_vp * max(n, 1))(*[None if p is None else p.handle for p in proofs])
    out = C.c_void_p()
    _check(nova_lib.vdf_nova_compress_aggregate(pp.handle, n, hs, C.byref(out)))
    return AggregateProof(out.value, pp)


def deserialize_aggregate(pp: NovaVDFPublicParams, data: bytes) -> AggregateProof:
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    h = C.c_void_p()
    _check(nova_lib.vdf_nova_aggregate_deserialize(pp.handle, buf, len(data), C.byref(h)))
    return AggregateProof(h.value, pp)


def aggregate_fold_instances(field_of_primary: int, side: int, digest: bytes, instances: Sequence[bytes], comm_TT: Sequence[bytes]):
    """The verifier's transcript and folds of one side over plain bytes, on the host alone (vdf_nova_aggregate_fold_instances).
    instances: 160-byte wire instances (comm_W | comm_E | u | X0 | X1); comm_TT: len(instances) - 1 32-byte points.  Returns
    (the folded instance's 160 bytes, the challenges as 32-byte Montgomery elements of the side's field)."""
    if len(digest) != 32:
        raise ValueError("instances are 160 bytes, points and the digest 32")
    n, inst, tt = _wire_instances(instances, comm_TT)
    dg = (C.c_uint8 * 32).from_buffer_copy(digest)
    acc = (C.c_uint8 * 160)()
    r = (C.c_uint8 * max(32 * (n - 1), 1))()
    _check(nova_lib.vdf_nova_aggregate_fold_instances(field_of_primary, side, dg, n, inst, tt, acc, r))
    return bytes(acc), [bytes(r[32 * k:32 * k + 32]) for k in range(max(n - 1, 0))]


def aggregate_fold_instances_device(pp: NovaVDFPublicParams, side: int, instances: Sequence[bytes], comm_TT: Sequence[bytes]):
    """aggregate_fold_instances with the points decoded and summed on the GPU (vdf_nova_aggregate_fold_instances_device); the
    orientation and the digest are pp's.  Returns the same (folded instance, challenges), byte for byte."""
    n, inst, tt = _wire_instances(instances, comm_TT)
    acc = (C.c_uint8 * 160)()
    r = (C.c_uint8 * max(32 * (n - 1), 1))()
    _check(nova_lib.vdf_nova_aggregate_fold_instances_device(pp.handle, side, n, inst, tt, acc, r))
    return bytes(acc), [bytes(r[32 * k:32 * k + 32]) for k in range(max(n - 1, 0))]


def verify_aggregate_wire(pp: NovaVDFPublicParams, data: bytes, num_steps: Sequence[int], z0: Sequence[Sequence[bytes]],
                          zi: Sequence[Sequence[bytes]]):
    """A verifier that holds bytes only (vdf_nova_verify_aggregate_wire): "VDFAGG01" in, (ok, bad_entry, decode_code) out.  Every
    point is decoded on the GPU and the device verifier runs; decode_code is deserialize_aggregate's error code for these bytes
    (0: they decode), and anything but 0 gives ok = False."""
    n, steps, z0a, zia = _aggregate_statements(pp, num_steps, z0, zi)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    ok, bad, code = C.c_int(0), C.c_int64(-1), C.c_int(0)
    _check(nova_lib.vdf_nova_verify_aggregate_wire(pp.handle, buf, len(data), n, steps, z0a, zia, C.byref(ok), C.byref(bad), C.byref(code)))
    return bool(ok.value), int(bad.value), int(code.value)


def aggregate_verify_times() -> list:
    """ms of the last device / wire verification on this thread: [exact checks (hashes), secondary folds, accumulators, arguments,
    decoding] (vdf_nova_aggregate_verify_times)."""
    ms = (C.c_double * 5)()
    _check(nova_lib.vdf_nova_aggregate_verify_times(ms))
    return list(ms)
