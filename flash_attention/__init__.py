"""Drop-in alias: `import flash_attention` resolves to the MI355X build."""
from flash_attention_from_scratch_amd.flash_attention import (  # noqa: F401
    append_kvcache, attention, attention_varlen, attention_varlen_sinks, backward, backward_varlen, backward_varlen_sinks,
    backward_varlen_softcap, backward_varlen_window, forward, forward_ex, forward_kvcache, forward_kvcache_softcap, forward_timed,
    forward_varlen, forward_varlen_kvcache, forward_varlen_sinks, quantize_kvcache_fp8,
)
