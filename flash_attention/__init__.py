"""Drop-in alias: `import flash_attention` resolves to the MI355X build."""
from flash_attention_from_scratch_amd.flash_attention import (  # noqa: F401
    append_kvcache, attention, attention_varlen, attention_varlen_sinks, backward, backward_varlen, backward_varlen_sinks,
    backward_varlen_softcap, backward_varlen_window, forward, forward_ex, forward_kvcache, forward_kvcache_d64, forward_kvcache_sinks,
    forward_kvcache_softcap, forward_timed, forward_varlen, forward_varlen_kvcache, forward_varlen_kvcache_sinks, forward_varlen_sinks,
    forward_varlen_d64, forward_varlen_kvcache_d64, kvcache_d64_num_splits, quantize_kvcache_fp8,
    attention_varlen_d64, backward_varlen_d64, forward_kvcache_d256, kvcache_d256_num_splits,
    forward_varlen_d256, forward_varlen_kvcache_d256,
)
