from locotouch_amd.rl.modules import ActorCritic, ActorCriticEncoder, ActorCriticRecurrent, ActorCriticRNNEncoder
from locotouch_amd.rl.normalizer import EmpiricalNormalization

__all__ = ["ActorCritic", "ActorCriticRecurrent", "ActorCriticEncoder", "ActorCriticRNNEncoder", "EmpiricalNormalization"]
