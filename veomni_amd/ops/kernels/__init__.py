from . import attention, cross_entropy, load_balancing_loss, moe, norms  # noqa: F401
