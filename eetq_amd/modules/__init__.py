from .qlinear import (EetqLinear, EetqLinearMMFunction, EetqSparseMoeBlock, EetqTopKRouter, W4A16Experts, W8A16Experts, W8A16Linear,  # noqa: F401
                      quantize_and_preprocess_weights)
